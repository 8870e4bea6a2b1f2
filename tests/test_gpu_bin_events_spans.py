"""mhi_bin_events where one workgroup walks SEVERAL chunks: spans of 2, 4 and 8 (the production path; every shape of
tests/test_gpu_bin_events.py ends at span 1).

The span is reached through the public call alone, by the choice of C and T; span_of() restates the library's rule and
every test asserts the span it claims with it -- a coverage guard, never an expectation: a retuned heuristic makes these
tests fail and say so, where they would otherwise quietly test span 1 again.  The expectations are the NumPy yardstick
of test_gpu_bin_events.py (counts_of, pack, Layout.image), byte for byte over the whole canary buffer, in all five
layouts.

    C      T              chunks  span  spans
    1366   4 * 16384 + 9  5       2     3      the last span holds one chunk, the cut one of 9 bins
    2048   4 * 16384 + 9  5       4     2      the second span starts with a search past four chunks
    4096   2 * 16384 + 7  3       8     1      the span is cut from 8 to 3 chunks; one workgroup walks a whole channel

Most channels are sparse filler; a handful, spread over low, middle and last channel indices, carry what a multi-chunk
walk can get wrong (Scene below).  A workgroup at span 2 holds two chunks, so "populated, empty, populated" inside ONE
workgroup exists at spans 4 and 8 only; at span 2 it is populated -> empty and empty -> populated.

Not reached: the library's second rule, which WIDENS the span when C x spans would exceed 2^31 - 1 workgroups, needs
more than 2^31 chunks in all and so no test-sized shape gets there."""
import numpy as np
import pytest

from tests import test_gpu_bin_events as be

pytestmark = pytest.mark.gpu

CH, LAYOUTS = be.CH, be.LAYOUTS
mh = be.mh          # the fixture: builds the ingest library, asserts a gfx950 device

# (C, T, period): periods 1, 30 and 2^18 are the kernel's three ways to divide
CASES = [(1366, 4 * CH + 9, 7), (2048, 4 * CH + 9, 30), (4096, 2 * CH + 7, 1), (4096, 2 * CH + 7, 30),
         (4096, 2 * CH + 7, 1 << 18)]
SPANS = {(1366, 4 * CH + 9): (2, 3), (2048, 4 * CH + 9): (4, 2), (4096, 2 * CH + 7): (8, 1)}


def span_of(C, T):
    """-> (chunks per workgroup, workgroups per channel): the rule of mhi_bin_events (csrc/mh_ingest.hip), restated"""
    n = -(-T // CH)
    span = 8
    while span > 1 and C * -(-n // span) < 4096:
        span >>= 1
    while C * -(-n // span) > 0x7FFFFFFF:
        span <<= 1
    return span, -(-n // span)


def test_the_shapes_reach_spans_2_4_and_8_and_the_other_file_does_not():
    assert {span_of(C, T)[0] for C, T, _ in CASES} == {2, 4, 8}
    for C, T in ((5, 2 * CH + 7), (6, 3 * CH + 11), (70, 147461), (4, 2 * CH + 100), (3, CH + 17)):
        assert span_of(C, T)[0] == 1


class Scene:
    """C channels of events for T bins of `period` ticks: filler, and the crafted channels in self.crafted
    (name -> channel).  check_inputs(counts) asserts in plain Python that every crafted channel IS its case."""

    FILL = 300

    def __init__(self, C, T, period, unsorted=True):
        self.C, self.T, self.period = C, T, period
        self.origin = origin = 1_000_003
        self.span, self.nspans = span_of(C, T)
        self.nch = nch = -(-T // CH)
        self.end = end = origin + T * period
        span = self.span
        rng = np.random.default_rng([C, T, period % 1009])
        fill = np.sort(rng.integers(origin - 50, end + 50, size=(C, self.FILL), dtype=np.int64), axis=1).astype(np.uint64)
        self.chans = list(fill)

        def at(bins, n=1):
            """n (one number, or one per bin) ticks in each of the ascending `bins`, spread over the bin's ticks, in order"""
            bins = np.asarray(bins, np.int64).reshape(-1)
            n = np.broadcast_to(np.asarray(n, np.int64), bins.shape)
            b, nn = np.repeat(bins, n), np.repeat(n, n)
            rank = np.arange(b.size, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
            return origin + b * period + rank * period // nn

        def chunk(j):
            return np.arange(j * CH, min((j + 1) * CH, T), dtype=np.int64)

        def sparse(j):
            b = chunk(j)
            return np.unique(np.concatenate([b[::97], b[:1], b[-1:]]))

        before, after = np.array([origin - 7, origin - 1], np.int64), np.array([end, end + 3], np.int64)
        pairs = [(j, j + 1) for j in range(nch - 1) if j // span == (j + 1) // span]           # two chunks of one workgroup
        full = [p for p in pairs if (p[1] + 1) * CH <= T]                                      # ... the second one not cut
        assert pairs and full
        first, last = full[0], full[-1]
        made, checks = [], []

        def add(name, parts, check):
            made.append((name, np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in parts]).astype(np.uint64)))
            checks.append((name, check))

        def nonzero_bins(row, j):
            return int(np.count_nonzero(row[j * CH:(j + 1) * CH]))

        # 1. a tile left over: chunk j full (one per bin, then saturated for each width), chunk j + 1 sparse
        def leftover(name, pair, n):
            j, k = pair
            want = np.broadcast_to(np.asarray(n, np.int64), (CH,))
            add(name, [before, at(chunk(j), n), at(sparse(k)), after],
                lambda row: (row[j * CH:k * CH] == want).all() and nonzero_bins(row, k) == len(sparse(k))
                and row[k * CH:(k + 1) * CH].max() == 1)
        m16 = np.arange(CH) % 16
        leftover("one per bin -> sparse", last, 1)
        leftover("4 per bin -> sparse", first, 4)                                              # the 2-bit cap in every bin
        leftover("16 in every 16th bin -> sparse", last, np.where(m16 == 3, 16, 1))            # the 4-bit cap in every vector
        leftover("256 in every 16th bin -> sparse", first, np.where(m16 == 11, 256, 1))        # the 8-bit cap in every vector

        # 2. chunks without events between and behind populated ones
        tri = [j for j in range(nch - 2) if j // span == (j + 2) // span]
        pop, emp = ((tri[-1], tri[-1] + 2), (tri[-1] + 1,)) if tri else ((0, 3), (1, 2))
        add("populated, empty, populated", [before] + [at(chunk(j)[::5], 2) for j in pop] + [after],
            lambda row: all(nonzero_bins(row, j) == len(chunk(j)[::5]) for j in pop)
            and not any(nonzero_bins(row, j) for j in emp))
        j = nch - 3
        add("populated, empty, empty and cut", [before, at(chunk(j)[::3]), after],
            lambda row, j=j: row[:j * CH].sum() == 0 and nonzero_bins(row, j) > 5000 and row[(j + 1) * CH:].sum() == 0)

        # 3. runs and exactly-full passes that end where the workgroup's next chunk begins
        for name, (j, k) in (("70000 | 70000", pairs[0]), ("70000 | 70000, later", pairs[-1])):
            add(name, [at([5], 1), at([k * CH - 1, k * CH], 70000), after],
                lambda row, k=k: row[k * CH - 1] == 70000 and row[k * CH] == 70000 and row.sum() == 140001)
        for n, pair, then in ((256, last, True), (256, first, False), (512, first, True), (512, last, False)):
            j, k = pair
            add("%d end chunk %d, the next %s" % (n, j, "populated" if then else "empty"),
                [before, at([5], 1) if j else [], at([k * CH - 1], n), at(sparse(k)) if then else [], after],
                lambda row, j=j, k=k, n=n, then=then: row[k * CH - 1] == n and row[j * CH:k * CH].sum() == n
                and nonzero_bins(row, k) == (len(sparse(k)) if then else 0))
        j, k = last
        add("256 bins end chunk", [before, at(chunk(j)[-256:]), at(sparse(k)), after],
            lambda row, j=j, k=k: row[j * CH:k * CH].sum() == 256 and (row[k * CH - 256:k * CH] == 1).all()
            and nonzero_bins(row, k) == len(sparse(k)))

        # 4. the start search of a later span, and a channel that lives in the last chunk only
        if self.nspans > 1:
            b0 = span * CH                                                                    # first bin of the second span
            ts = origin + b0 * period
            add("search", [before, at(np.arange(14000), 5), [ts - 1] * 3, [ts] * 3, at([b0 + 1, b0 + 5, T - 1]), after],
                lambda row: row[:b0 - 1].sum() == 70000 and row[b0 - 1] == 3 and row[b0] == 3 and row[b0 + 1] == 1
                and row[T - 1] == 1)
        add("last chunk only", [origin - 1 - np.arange(300)[::-1], at(chunk(nch - 1), 2), end + np.arange(300)],
            lambda row: row[:(nch - 1) * CH].sum() == 0 and (row[(nch - 1) * CH:] == 2).all())

        # 5. nothing to do
        nothing = lambda row: row.sum() == 0      # noqa: E731
        add("no events", [[]], nothing)
        add("only before origin", [origin - 1 - np.arange(500)[::-1]], nothing)
        add("only at or past the end", [end + np.arange(500)], nothing)

        # 6. one channel in descending order
        self.skip = ()
        if unsorted:
            add("unsorted", [np.sort(rng.integers(origin - 50, end + 50, size=5000, dtype=np.int64))[::-1]],
                lambda row: row.sum() > 4900)

        # low, middle and last channel indices in turn: blockIdx.x / nspans and % nspans see small and large values
        third = -(-len(made) // 3)
        slots = [c for k in range(third) for c in (k, C // 2 - third // 2 + k, C - 1 - k)]
        assert len(set(slots)) == len(slots) and min(slots) == 0 and max(slots) == C - 1
        self.crafted = {}
        for (name, ticks), c in zip(made, slots):
            assert name not in self.crafted
            self.crafted[name] = c
            self.chans[c] = ticks
            if name != "unsorted":
                assert (np.diff(ticks.astype(np.int64)) >= 0).all(), name
        if unsorted:
            self.skip = (self.crafted["unsorted"],)
        self.checks = checks

    def check_inputs(self, counts):
        assert len(self.crafted) >= 17 + (self.nspans > 1)
        for name, check in self.checks:
            assert check(counts[self.crafted[name]]), (name, self.crafted[name])
        c = self.crafted.get("search")
        if c is not None:     # three rounds of the 256-ary search: more than 256^2 events before the span's first tick
            assert int((self.chans[c] < np.uint64(self.origin + self.span * CH * self.period)).sum()) > 65536


def locate(lay, byte):
    """-> (channel or None, text): the channel, chunk and bin behind a byte of the buffer, for the assertion message"""
    per = 8 // lay.bits
    if lay.bits == 8:
        c, r = divmod(byte - 203, lay.T + 37)
        b = r if r < lay.T else None
    elif not lay.blocked:
        nbytes = (lay.T + 15) // 16 * 2 * lay.bits
        c, r = divmod(byte - 256, int(lay.off[1] - lay.off[0]) if lay.C > 1 else lay.size)
        b = r * per if r < nbytes else None
    else:
        cb = CH * lay.bits // 8
        j, r = divmod(byte - 256, lay.stride)
        c, r = divmod(r, cb)
        b = j * CH + r * per
    if byte < int(lay.off[0]) or not 0 <= c < lay.C or b is None or b >= (lay.T + 15) // 16 * 16:
        return None, "outside every channel"
    return c, "channel %d, chunk %d, bin %d of it%s" % (c, b // CH, b % CH, "" if per == 1 else " and the %d after" % (per - 1))


def compare(mh, scene, ev, counts, bits, blocked):
    lay, buf, rc = be.run(mh, ev, scene.origin, scene.period, scene.T, bits, blocked)
    assert rc == 0, mh._ingest.lib().mhi_last_error()
    want, mask = lay.image(counts, scene.skip)
    got = buf.cpu().numpy()
    bad = np.flatnonzero((got != want) & mask)
    if bad.size:
        c, text = locate(lay, int(bad[0]))
        name = {v: k for k, v in scene.crafted.items()}.get(c, "filler")
        raise AssertionError("span %d, bits %d, %s: first differing byte %d of %d: got %d, want %d, %s [%s]; %d bytes differ"
                             % (scene.span, bits, "chunk-blocked" if blocked else "contiguous", bad[0], lay.size, got[bad[0]],
                                want[bad[0]], text, name, bad.size))


@pytest.fixture(scope="module", params=CASES, ids=lambda p: "C%d-T%d-p%d" % p)
def scene(request, mh):
    """one scene per (C, T, period), shared by the five layouts: the events on the device and their NumPy counts"""
    C, T, period = request.param
    sc = Scene(C, T, period)
    assert (sc.span, sc.nspans) == SPANS[(C, T)] == span_of(C, T)
    counts = be.counts_of(sc.chans, sc.origin, period, T)
    sc.check_inputs(counts)
    e = be.Events(mh, sc.chans)
    yield sc, e.ev, counts
    del e, counts


@pytest.mark.parametrize("bits,blocked", LAYOUTS)
def test_spans_of_2_4_and_8_chunks(mh, scene, bits, blocked):
    sc, ev, counts = scene
    assert span_of(sc.C, sc.T) == SPANS[(sc.C, sc.T)] and sc.span > 1
    compare(mh, sc, ev, counts, bits, blocked)


# ---- through the stack, at span 8 ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack(mh):
    C, T, period = 4096, 2 * CH + 7, 30
    assert span_of(C, T) == (8, 1)
    sc = Scene(C, T, period, unsorted=False)       # EventSet checks the order: every channel sorted here
    counts = be.counts_of(sc.chans, sc.origin, period, T)
    sc.check_inputs(counts)
    assert counts.max() >= 256
    return sc, np.minimum(counts, 255).astype(np.uint8)


def test_channel_set_from_events_at_span_8(mh, stack):
    from muahuff import container, events
    sc, binned = stack
    ev = events.EventSet.from_channels(sc.chans)
    cs = container.ChannelSet.from_events(ev, sc.origin, sc.period, sc.T)
    assert cs.C == sc.C and (cs.ch_len == sc.T).all()
    want = np.zeros(cs.data.numel(), np.uint8)      # the channels where the set puts them, zero padding everywhere else
    for c in range(sc.C):
        want[int(cs.ch_off[c]):int(cs.ch_off[c]) + sc.T] = binned[c]
    got = cs.data.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing byte %d: got %d, want %d; %d differ" % (bad[0], got[bad[0]], want[bad[0]], bad.size)


@pytest.mark.parametrize("S", [3, 5])
def test_stream_encoder_from_events_equals_the_block_path_at_span_8(mh, stack, S):
    """S = 3: 2-bit chunk-blocked pieces, S = 5: 4-bit; the body of the span-1 test in test_gpu_bin_events.py"""
    sc, binned = stack
    assert span_of(sc.C, sc.T) == (8, 1) and binned.max() >= S
    be.stream_events_equal_block(sc.chans, binned, sc.origin, sc.period, S, sc.T, host_form=False)
