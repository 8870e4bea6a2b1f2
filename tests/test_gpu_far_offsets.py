"""Every entry point of both libraries with an offset, a pitch or a stride beyond 4 GiB: the cases of tests/far_offsets.py
on the device.  The windows of a case's `pre` image -- around every true region and around every alias, where a 32-bit
cut of the offset or of a product would land -- are uploaded into an arena that is otherwise never touched, the call is
made with direct ctypes calls on the arena's base pointer (the Python wrappers would copy or re-lay-out the data), and
every window is downloaded and compared WHOLE with the `post` image: the yardstick's result inside canary at the far
place, the low place exactly as it was.  Return codes, status words and the small outputs are asserted by the case's own
`run`.  tests/test_host_far_offsets.py shows without a GPU that no address of any case, cut or not, leaves the arena.

The two arenas come from torch.empty: 2^32 + 2^28 bytes for the module, and 4 * (2^32 + 2^26) bytes for the three
word-indexed cases alone, freed right after them."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

from tests import far_offsets as fo

pytestmark = pytest.mark.gpu

_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
          np.dtype(np.int64): torch.int64, np.dtype(np.uint64): torch.int64, np.dtype(np.float64): torch.float64}


def _need(nbytes, what):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    assert nbytes < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (what, nbytes / 1e9, free / 1e9)


class Ctx:
    """what a case's run() gets: the libraries, the arena and the little helpers of a direct ctypes call"""

    def __init__(self, mh, arena):
        self.mh, self.arena, self.base = mh, arena, arena.data_ptr()
        self.bytes = arena if arena.dtype == torch.uint8 else arena.view(torch.uint8)
        self.words = arena if arena.dtype == torch.int32 else arena.view(torch.int32)
        self.lib, self.ilib = mh._lib.lib(), mh._ingest.lib()
        self.keep = []

    def at(self, addr):
        assert 0 <= addr < self.arena.numel() * self.arena.element_size()
        return ct.c_void_p(self.base + addr)

    def dev(self, a):
        a = np.ascontiguousarray(a)
        view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        t = torch.from_numpy(a.view(view) if view else a).cuda()
        self.keep.append(t)
        return t

    def u64(self, a):
        return self.dev(np.asarray([int(v) for v in a], np.uint64))

    def p(self, t, skip=0):
        return None if t is None else ct.c_void_p(t.data_ptr() + skip * t.element_size())

    def canary(self, n, dtype):
        t = torch.full((n * np.dtype(dtype).itemsize,), fo.CANARY, dtype=torch.uint8, device="cuda").view(_TORCH[np.dtype(dtype)])
        self.keep.append(t)
        return t

    def host(self, t):
        a = t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def framed(self, t, lead, body, tag):
        """t (from canary()) holds `body` behind `lead` canary elements and canary behind it, bit for bit"""
        got = t.cpu().numpy().view(np.uint8)
        exp = np.full(got.size, fo.CANARY, np.uint8)
        b = fo.as_bytes(body)
        exp[lead * t.element_size():lead * t.element_size() + b.size] = b
        assert np.array_equal(got, exp), (tag, t.cpu().numpy(), body)

    def sync(self):
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def mh():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()
    import muahuff
    from muahuff import codec, container, sclv, sweep, windows  # noqa: F401
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    return muahuff


@pytest.fixture(scope="module")
def arena(mh):
    """2^32 + 2^28 bytes, never filled as a whole"""
    _need(fo.ARENA_BYTES + fo.HEADROOM, "the arena of 2^32 + 2^28 bytes (+ 2 GiB for the small tensors)")
    a = torch.empty(fo.ARENA_BYTES, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arena_w(mh):
    """2^32 + 2^26 int32 words for the word-indexed cases; freed when they are done"""
    _need(fo.ARENA_W_BYTES + fo.HEADROOM, "arena W of 4 * (2^32 + 2^26) bytes (+ 2 GiB for the small tensors)")
    a = torch.empty(fo.ARENA_W_WORDS, dtype=torch.int32, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def _bytes(t):
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def run_case(mh, arena, case):
    s = case.setup()
    flat = _bytes(arena)
    assert flat.numel() == s.pre.size
    for lo, buf, _mark in s.pre.wins:
        flat[lo:lo + buf.size].copy_(torch.from_numpy(buf))
    ctx = Ctx(mh, arena)
    torch.cuda.synchronize()
    s.run(ctx)
    torch.cuda.synchronize()
    assert len(s.post.wins) == len(s.pre.wins)
    for lo, exp, _mark in s.post.wins:
        got = flat[lo:lo + exp.size].cpu().numpy()
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            i = int(bad[0])
            pytest.fail("%s: window [%#x, %#x): %d bytes differ, the first at %#x: got %#x, want %#x"
                        % (case.id, lo, lo + exp.size, bad.size, lo + i, int(got[i]), int(exp[i])))


def _row(row, arena="A"):
    cases = [c for c in fo.CASES if c.row == row and c.arena == arena]
    assert cases, row
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


@_row("codec")
def test_byte_plan_codec(mh, arena, case):
    run_case(mh, arena, case)


@_row("packed")
def test_packed_plans_and_the_packed_binner(mh, arena, case):
    run_case(mh, arena, case)


@_row("range")
def test_decode_range_and_decode_rebin(mh, arena, case):
    run_case(mh, arena, case)


@_row("rebin")
def test_rebin(mh, arena, case):
    run_case(mh, arena, case)


@_row("transpose")
def test_deinterleave_and_interleave(mh, arena, case):
    run_case(mh, arena, case)


@_row("synth")
def test_synth_poisson(mh, arena, case):
    run_case(mh, arena, case)


@_row("sweep")
def test_sweep(mh, arena, case):
    run_case(mh, arena, case)


@_row("analysis")
def test_reduce_rows_and_power_draws(mh, arena, case):
    run_case(mh, arena, case)


@_row("bin8")
def test_bin_events_bytes(mh, arena, case):
    run_case(mh, arena, case)


@_row("crc")
def test_seg_crc32(mh, arena, case):
    run_case(mh, arena, case)


@_row("unbin")
def test_unbin_csr(mh, arena, case):
    run_case(mh, arena, case)


@_row("excess")
def test_excess_rows(mh, arena, case):
    run_case(mh, arena, case)


@_row("apply")
def test_excess_apply(mh, arena, case):
    run_case(mh, arena, case)


@_row("windows")
def test_windows(mh, arena, case):
    run_case(mh, arena, case)


@_row("gram")
def test_gram(mh, arena, case):
    run_case(mh, arena, case)


# the 16-GiB arena is allocated for these three alone: a test function of their own keeps the rest of the file quick
_W = [c for c in fo.CASES if c.arena == "W"]


@pytest.mark.parametrize("case", _W, ids=[c.id for c in _W])
def test_word_offsets_beyond_2_32_words(mh, arena_w, case):
    run_case(mh, arena_w, case)
