"""Two calls that cover what a user of the reference usually wants.

bit_rates(...)   per-channel bit rate exactly as the reference's scripts compute it for one
                 design point (get_BR_with_approx_sort.py:164-193, 281-292): clip at S,
                 calibrate on the first 2^hist_bits bins, map (approx-sort or identity), pick
                 the best of the given static Huffman encoders, measure the next T/2 bins;
                 BR = 1000 / (BP / (bits / n)) in bits/s/channel, NaN for skipped channels.
compress(...)    the same design point, but actually emitting the bitstream (container_io).
"""
import numpy as np


def bit_rates(channels, S=3, hist_bits=6, approx=True, sclv_rows=None, BP=50):
    """channels: list of 1-D count arrays (or a ChannelSet).  Returns dict with BR (float64
    [C]), bits, n, enc, peak, skipped -- all host arrays."""
    import torch

    from . import MODE_APPROX, MODE_NOSORT, WIN_REF_HALF, codec, sclv
    from .container import ChannelSet
    cs = channels if isinstance(channels, ChannelSet) else ChannelSet.from_channels(channels)
    rows = sclv.table(S) if sclv_rows is None else np.asarray(sclv_rows, dtype=np.uint8).reshape(-1, S)
    plan = codec.Plan(cs.ch_off, cs.ch_len, S, hist_bits, MODE_APPROX if approx else MODE_NOSORT, WIN_REF_HALF, rows)
    m = plan.measure(cs.data)
    torch.cuda.synchronize()
    bits = m.bits.cpu().numpy().astype(np.float64)
    n = m.post_hist.sum(1).cpu().numpy().astype(np.float64)
    out = dict(BR=codec.bit_rate(bits, n, BP), bits=bits.astype(np.int64), n=n.astype(np.int64),
               enc=m.enc.cpu().numpy(), peak=m.peak.cpu().numpy(), skipped=m.skipped.cpu().numpy())
    plan.close()
    return out


def compress(channels, S=3, hist_bits=6, approx=True, sclv_rows=None, path=None, checksum=False, exact=False):
    """Encode everything after the calibration window of every channel.  Returns a
    container_io.Compressed (and writes it to `path` when given).  checksum=True: a revision-4 container that carries
    the CRC-32 of every segment, taken on the device and verified there whenever the container is read.
    exact=True: the container also keeps, as a sparse list, every sample the clip at S-1 cut (container_io.compress): the
    stream is unchanged, `c.excess_bits` is the price, and decompress() then returns the counts themselves."""
    from . import MODE_APPROX, MODE_NOSORT, container_io, sclv
    from .container import ChannelSet
    cs = channels if isinstance(channels, ChannelSet) else ChannelSet.from_channels(channels)
    rows = sclv.table(S) if sclv_rows is None else np.asarray(sclv_rows, dtype=np.uint8).reshape(-1, S)
    c = container_io.compress(cs, S, hist_bits, MODE_APPROX if approx else MODE_NOSORT, rows, checksum=checksum, exact=exact)
    if path is not None:
        container_io.save(path, c)
    return c


def decompress(c_or_path, channels=None, start=None, stop=None, bin=None, exact=None):
    """-> list of uint8 arrays: min(x, S-1) after the calibration window, zeros before it.
    channels: optional list of channel indices to decode (random access through the directory).
    start / stop (either given): only samples [start, stop) of each channel (defaults 0 and the longest channel's
    length), zero past a channel's end; a path is then opened with container_io.open, so only the header, the
    directory and the payload of the segments that overlap the range are read.
    bin=r: the same samples summed in bins of r (uint8, saturating at 255 as rebin_u8), decoded in one pass that never
    stores the fine samples (container_io.decompress_binned).  Without a range channel i gets its own ceil(T_i / r)
    bins; with one every row has ceil((stop - start) / r), and start must be a multiple of r.
    A path that holds a recording archive (archive.py) is answered from the archive: rows of global samples [start,
    stop) (defaults 0 and the archive's T) across its blocks, the same shapes as for a container.
    exact: None = a source written with exact=True gives the counts themselves (its excess lists are added back), any
    other min(x, S-1); False = never read the lists; True = ValueError when the source has none."""
    from . import container_io
    kw = {} if exact is None else {"exact": exact}      # None is every reader's default
    is_path = isinstance(c_or_path, (str, bytes)) or hasattr(c_or_path, "__fspath__")
    if is_path:
        from . import archive
        if archive.is_archive(c_or_path):
            with archive.open(c_or_path) as a:
                host = a.read(0 if start is None else int(start), a.T if stop is None else int(stop), channels=channels,
                              bin=None if bin is None else int(bin), **kw).cpu().numpy()
            return [row.copy() for row in host]
    if bin is not None:
        r = int(bin)

        def binned(src):
            host = container_io.decompress_binned(src, r, 0 if start is None else int(start),
                                                  None if stop is None else int(stop), channels=channels, **kw).cpu().numpy()
            if start is not None or stop is not None:
                return [row.copy() for row in host]
            sel = range(len(src.ch_len)) if channels is None else channels
            return [row[:(int(src.ch_len[c]) + r - 1) // r].copy() for row, c in zip(host, sel)]
        if is_path:
            with container_io.open(c_or_path) as f:
                return binned(f)
        return binned(c_or_path)
    if start is None and stop is None:
        c = container_io.load(c_or_path) if is_path else c_or_path
        return container_io.decompress(c, channels=channels, **kw).to_channels()

    def rows(src):
        lo = 0 if start is None else int(start)
        hi = int(np.max(src.ch_len)) if stop is None else int(stop)
        host = container_io.decompress_range(src, lo, hi, channels=channels, **kw).cpu().numpy()
        return [r.copy() for r in host]
    if is_path:
        with container_io.open(c_or_path) as f:
            return rows(f)
    return rows(c_or_path)
