"""The ingest kernels where the AMOUNT of data carries an index past 2^32: the cases of tests/big_inputs.py on the device,
at FAR = 2^32.  tests/test_host_big_inputs.py shows without a GPU that every closed form used here is the brute-force
model's result, that it differs from what an index cut to 32 bits would give, and that no cut index leaves an allocation.

  Wrong, never a fault.  Every index starts at its buffer's first element, so an index cut modulo 2^32 lands in the same
  buffer: a narrowed kernel reads a decoy or leaves canary, and the comparison fails.
  Lead.  A buffer that is walked through [2^31, 2^32) starts 2^31 bytes inside its allocation, canary in front: a
  sign-extended 32-bit byte offset stays inside the allocation.  Where the buffer is an output the lead is compared; where it
  is an input a read of the lead shows as counts that nobody planted.
  Memory.  Each case asserts its computed peak (big_inputs.Built.peak) against the free memory before it allocates, and
  everything is freed behind it.
  On the device.  Inputs and large expectations are built there -- repeat, arange, repeat_interleave, indexed assignment of
  the planted entries -- and compared there; the small tables and the planted neighbourhoods come back to the host.

Every comparison is exact."""
import gc
import importlib
import time
import types

import numpy as np
import pytest
import torch

from tests import big_inputs as bi

pytestmark = pytest.mark.gpu

FAR = 1 << 32
CHUNK = 1 << 26          # elements of one piece of a chunked comparison


@pytest.fixture(scope="module")
def ing():
    importlib.import_module("hardware-efficient-mua-compression_amd.build").build_ingest()
    import muahuff
    from muahuff import _ingest
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    assert "gfx950" in muahuff.device_info(0)["arch"]
    torch.cuda.set_device(0)
    return _ingest


@pytest.fixture(autouse=True)
def freed(request):
    """nothing of a case outlives it; what it allocated -- on top of what earlier modules of the same process still
    hold -- stays below its computed peak; its wall time is printed (pytest -s), never asserted"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    print("\n[big-inputs] %s: %.2f s, peak %.2f GB allocated" % (request.node.name, time.perf_counter() - t0, peak / 1e9))
    gc.collect()
    torch.cuda.empty_cache()
    computed, _COMPUTED[0] = _COMPUTED[0], 0
    assert computed == 0 or peak <= computed, "allocated %.2f GB, computed peak %.2f GB" % (peak / 1e9, computed / 1e9)


_COMPUTED = [0]          # the computed peak of the case that runs, for `freed`


def _build(cid):
    b = bi.BY_ID[cid].build(FAR)
    _COMPUTED[0] = b.peak
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    assert b.peak < free, "%s needs ~%.1f GB of free HBM; %.1f GB free" % (cid, b.peak / 1e9, free / 1e9)
    return b, b.shape


def _led(body_bytes, fill=bi.CANARY):
    """(allocation, body): the body begins LEAD bytes inside the allocation, canary in front of it"""
    whole = torch.empty(bi.LEAD + body_bytes, dtype=torch.uint8, device="cuda")
    whole[:bi.LEAD] = bi.CANARY
    whole[bi.LEAD:] = fill
    return whole, whole[bi.LEAD:]


def _lead_intact(whole):
    return bool((whole[:bi.LEAD].view(torch.int64) == bi.CAN64).all())


def _i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64, device="cuda")


def _canary(n, dtype):
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), bi.CANARY, dtype=torch.uint8, device="cuda").view(dtype)


def _plant(body, planted, base=0):
    idx = _i64([base + i for i, _v in planted])
    body[idx] = torch.tensor([v for _i, v in planted], dtype=torch.uint8, device="cuda")


def _host(t):
    return t.cpu().numpy().astype(np.int64)


def _is(t, want):
    got = _host(t)
    want = np.asarray(want, np.int64).reshape(got.shape)
    assert np.array_equal(got, want), (got, want)


def _rows(periods, reps, cols, pitch):
    x = torch.zeros((len(periods), pitch), dtype=torch.uint8, device="cuda")
    for i, p in enumerate(periods):
        x[i, :cols] = torch.from_numpy(np.ascontiguousarray(p)).cuda().repeat(reps)[:cols]
    return x


def _unbin_count(ing, form, x, row_off, rows, cols):
    ev_off = _canary(rows + 1, torch.int64) if form == ing.UNBIN_CSR else None
    total = _canary(1, torch.int64)
    scratch = torch.empty(ing.unbin_scratch_bytes(form, rows, cols), dtype=torch.uint8, device="cuda")
    ing.unbin_count(form, x, row_off, rows, cols, ev_off, total, scratch)
    torch.cuda.synchronize()
    return ev_off, total, scratch


# ---- the un-binner ---------------------------------------------------------------------------------------------------------
def test_unbin_far_out(ing):
    """out_ticks past byte 2^32: 3 rows of a 256-byte pattern holding every count once, 2^29 + 4099 events and more.  The
    whole output against torch.repeat_interleave, the neighbourhood of entry 2^29 against the closed form, canary behind
    `total` and in the lead."""
    b, s = _build("unbin-far-out")
    rows, cols, total = s["rows"], s["cols"], s["total"]
    x = _rows(b.inputs["period"], b.inputs["reps"], cols, s["pitch"])
    row_off = _i64([i * s["pitch"] for i in range(rows)])
    ev_off, tot, scratch = _unbin_count(ing, ing.UNBIN_CSR, x, row_off, rows, cols)
    _is(ev_off, b.expect["ev_off"])
    _is(tot, [total])
    whole, body = _led(8 * (total + s["tail"]))
    out = body.view(torch.int64)
    over = torch.zeros(1, dtype=torch.int64, device="cuda")
    ing.unbin_emit(ing.UNBIN_CSR, x, row_off, rows, cols, bi.ORIGIN, bi.PERIOD, bi.PHASE, out, None, over, scratch)
    torch.cuda.synchronize()
    _is(over, [0])
    tick = bi.ORIGIN + torch.arange(cols, dtype=torch.int64, device="cuda") * bi.PERIOD + bi.PHASE
    ev = [int(v) for v in b.expect["ev_off"]]
    for i in range(rows):                                      # row by row: a third of the expectation at a time
        want = torch.repeat_interleave(tick, x[i, :cols].to(torch.int64))
        assert want.numel() == ev[i + 1] - ev[i]
        assert torch.equal(out[ev[i]:ev[i + 1]], want), i
        del want
    e = np.concatenate([np.arange(300), np.arange(s["unit"] - 300, s["unit"] + 300), np.arange(total - 300, total)])
    _is(out[torch.from_numpy(e).cuda()], b.expect["ticks"](e))
    assert bool((out[total:] == bi.CAN64).all()) and _lead_intact(whole)


def test_unbin_dense_group(ing):
    """A group sum above 2^31: row 0 is all 255 for the whole first group of 1024 tiles (4 278 190 080 events), the
    largest value the scan's two 16-bit halves ever take.  ev_off and total exact; the emit pass into 2^16 entries: the
    first 2^16 ticks, over = total - 2^16, canary at and behind the capacity."""
    b, s = _build("unbin-dense-group")
    cols, cap = s["cols"], s["capacity"]
    x = _rows(b.inputs["period"], cols // 256, cols, s["pitch"])
    r, lo, hi, v = b.inputs["fill"]
    x[r, lo:hi] = v
    row_off = _i64([0, s["pitch"]])
    ev_off, tot, scratch = _unbin_count(ing, ing.UNBIN_CSR, x, row_off, 2, cols)
    _is(ev_off, b.expect["ev_off"])
    _is(tot, [b.expect["total"]])
    out = _canary(cap + bi.P, torch.int64)
    over = torch.zeros(1, dtype=torch.int64, device="cuda")
    ing.unbin_emit(ing.UNBIN_CSR, x, row_off, 2, cols, bi.ORIGIN, bi.PERIOD, bi.PHASE, out, None, over, scratch, capacity=cap)
    torch.cuda.synchronize()
    _is(out[:cap], b.expect["ticks"](np.arange(cap)))
    assert bool((out[cap:] == bi.CAN64).all())
    _is(over, [b.expect["over"]])
    assert b.expect["over"] == b.expect["total"] - (1 << 16)


def test_unbin_csr_long_row(ing):
    """A column >= 2^32 of one row: 2 rows of 2^32 + 4099 zeros with counts planted at columns 2^32 - 1 (the end of a
    tile), 2^32, 2^32 + d (a 255) and the last one, and decoys at the aliases."""
    b, s = _build("unbin-csr-long-row")
    cols, pitch = s["cols"], s["pitch"]
    whole, body = _led(2 * pitch, fill=0)
    for i, p in enumerate(b.inputs["planted"]):
        _plant(body, p, i * pitch)
    row_off = _i64([0, pitch])
    ev_off, tot, scratch = _unbin_count(ing, ing.UNBIN_CSR, body, row_off, 2, cols)
    _is(ev_off, b.expect["ev_off"])
    _is(tot, [b.expect["total"]])
    out = _canary(b.expect["total"] + 8, torch.int64)
    over = torch.zeros(1, dtype=torch.int64, device="cuda")
    ing.unbin_emit(ing.UNBIN_CSR, body, row_off, 2, cols, bi.ORIGIN, bi.PERIOD, bi.PHASE, out, None, over, scratch)
    torch.cuda.synchronize()
    _is(out, np.concatenate([b.expect["ticks"], [bi.CAN64] * 8]))
    _is(over, [0])
    assert not np.array_equal(b.expect["ticks"], b.cut["ticks"])


@pytest.mark.parametrize("ch_bits", [16, 32])
def test_unbin_aer_big_block(ing, ch_bits):
    """The flat element index >= 2^32 and the division f0 / cols behind it: a block of 1000 channels and 4294971 time
    steps (2^18 + 1 tiles), zeros with planted counts; ticks and channels."""
    b, s = _build("unbin-aer-big-block")
    rows, cols = s["rows"], s["cols"]
    whole, body = _led(s["n"], fill=0)
    _plant(body, b.inputs["planted"])
    _none, tot, scratch = _unbin_count(ing, ing.UNBIN_AER, body, None, rows, cols)
    total = b.expect["total"]
    _is(tot, [total])
    cdt = torch.int16 if ch_bits == 16 else torch.int32
    out, out_ch = _canary(total + 8, torch.int64), _canary(total + 8, cdt)
    over = torch.zeros(1, dtype=torch.int64, device="cuda")
    ing.unbin_emit(ing.UNBIN_AER, body, None, rows, cols, bi.ORIGIN, bi.PERIOD, bi.PHASE, out, out_ch, over, scratch)
    torch.cuda.synchronize()
    _is(out[:total], b.expect["ticks"])
    _is(out_ch[:total], b.expect["channels"])
    assert bool((out[total:] == bi.CAN64).all())
    assert bool((out_ch[total:].contiguous().view(torch.uint8) == bi.CANARY).all())
    _is(over, [0])


# ---- the partition ---------------------------------------------------------------------------------------------------------
def test_aer_far_out(ing):
    """Positions >= 2^29: more than 2^29 + 4099 pairs with ticks[i] = i over C = 3, one pair in a thousand dropped.  Channel
    1's run straddles byte 2^32 of out_ticks, channel 2's lies wholly behind it.  Every run against its closed form, in
    pieces, on the device."""
    b, s = _build("aer-far-out")
    n, C, L, kept = s["n"], s["C"], s["L"], s["kept"]
    pat = torch.from_numpy(b.inputs["period"].view(np.int16)).cuda()
    channels = pat.repeat(-(-n // L))[:n]
    assert channels.is_contiguous() and channels.numel() == n
    ticks = torch.arange(n, dtype=torch.int64, device="cuda")
    whole, body = _led(8 * (n + s["tail"]))
    out = body.view(torch.int64)
    ev_off, dropped = _canary(C + 1, torch.int64), _canary(1, torch.int64)
    scratch = torch.empty(ing.aer_scratch_bytes(n, C), dtype=torch.uint8, device="cuda")
    ing.aer_to_csr(ticks, channels, C, out, ev_off, dropped, scratch)
    torch.cuda.synchronize()
    del ticks, channels
    ev = b.expect["ev_off"]
    _is(ev_off, ev)
    _is(dropped, [b.expect["dropped"]])
    assert 8 * int(ev[1]) < FAR < 8 * int(ev[2])
    for c in range(C):
        pos = torch.from_numpy(b.inputs["positions"][c]).cuda()
        q, first, count = pos.numel(), int(ev[c]), int(ev[c + 1] - ev[c])
        for k0 in range(0, count, CHUNK):
            k = torch.arange(k0, min(k0 + CHUNK, count), dtype=torch.int64, device="cuda")
            want = torch.div(k, q, rounding_mode="floor") * L + pos[k % q]
            assert torch.equal(out[first + k0:first + k0 + k.numel()], want), (c, k0)
            del k, want
    p = np.concatenate([np.arange(300), np.arange(s["unit"] - 300, s["unit"] + 300), np.arange(kept - 300, kept)])
    _is(out[torch.from_numpy(p).cuda()], b.expect["ticks"](p))
    assert bool((out[kept:] == bi.CAN64).all()) and _lead_intact(whole)


# ---- the windows -----------------------------------------------------------------------------------------------------------
def test_windows_far_offsets(ing):
    """win_off >= 2^32: 2 rows of 2^32 + 8198 columns on an odd pitch, a pattern of period 4099 with the first 64 bytes of
    each row at 255; 12 windows of 200, six of them behind 2^32 and one ending exactly at `cols`.  STACK 8-bit, STACK 32-bit
    with win_idx and SUM with sumsq, each with r = 1, 7 and 100 (the lane, the staged and the wave kernel)."""
    b, s = _build("windows-far-offsets")
    cols, stride, W, n_win = s["cols"], s["stride"], s["W"], s["n_win"]
    whole, body = _led(2 * stride, fill=0)
    n_head, v_head = b.inputs["head"]
    for i, p in enumerate(b.inputs["period"]):
        row = body[i * stride:i * stride + cols]
        pt = torch.from_numpy(p).cuda()
        reps = cols // p.size
        row[:reps * p.size].view(reps, p.size).copy_(pt.expand(reps, p.size))
        row[reps * p.size:] = pt[:cols - reps * p.size]
        row[:n_head] = v_head
    win_off, win_idx = _i64(b.inputs["win_off"]), _i64(b.inputs["win_idx"])
    bad = ing.verify_state("cuda")
    x_ptr = body.data_ptr()
    for r in bi.WIN_R:
        nb = -(-W // r)
        out = _canary(n_win * 2 * nb, torch.uint8).view(n_win, 2, nb)
        ing.windows(x_ptr, stride, 2, cols, win_off, None, n_win, W, r, ing.WIN_STACK, out.data_ptr(), 8, 2 * nb, nb, bad)
        torch.cuda.synchronize()
        _is(out, b.expect["stack8", r])
        out = _canary(n_win * 2 * nb, torch.int32).view(n_win, 2, nb)
        ing.windows(x_ptr, stride, 2, cols, win_off, win_idx, n_win, W, r, ing.WIN_STACK, out.data_ptr(), 32, 8 * nb, 4 * nb, bad)
        torch.cuda.synchronize()
        _is(out, b.expect["stack32idx", r])
        out, sq = _canary(2 * nb, torch.int32).view(2, nb), _canary(2 * nb, torch.int64).view(2, nb)
        ing.windows(x_ptr, stride, 2, cols, win_off, None, 0, W, r, ing.WIN_SUM, out.data_ptr(), 32, 0, 4 * nb, bad,
                    sumsq=sq, sq_row_stride=8 * nb)
        torch.cuda.synchronize()
        _is(out, b.expect["sum", r][0])
        _is(sq, b.expect["sum", r][1])
    _is(bad, [0, -1])


def test_windows_many_items(ing):
    """win_split's 64-bit branch: 65537 rows x 65536 windows of one sample are 2^32 + 65536 items of the lane form.  Every
    row distinct, the offsets cycle through all 257 columns; the output [n_win, rows, 1], prefilled with canary, against
    x[:, off].t() whole, on the device."""
    b, s = _build("windows-many-items")
    rows, n_win, cols, pitch = s["rows"], s["n_win"], s["cols"], s["pitch"]
    i, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    x = torch.zeros((rows, pitch), dtype=torch.uint8, device="cuda")
    x[:, :cols] = torch.from_numpy(b.inputs["val"](i, c).astype(np.uint8)).cuda()
    off = torch.arange(n_win, dtype=torch.int64, device="cuda") % cols
    _is(off[:600], b.inputs["win_off"](np.arange(600)))
    whole, out = _led(s["items"])
    bad = ing.verify_state("cuda")
    ing.windows(x.data_ptr(), pitch, rows, cols, off, None, n_win, 1, 1, ing.WIN_STACK, out.data_ptr(), 8, rows, 1, bad)
    torch.cuda.synchronize()
    xt, got = x[:, :cols].t().contiguous(), out.view(n_win, rows)
    for k0 in range(0, n_win, n_win // 4):                     # x[:, off].t(), a quarter of the windows at a time
        want = xt[off[k0:k0 + n_win // 4]]
        assert want.is_contiguous() and torch.equal(got[k0:k0 + n_win // 4], want), k0
        del want
    k, r = np.array([0, 1, n_win - 1, n_win - 1, n_win - 1]), np.array([0, rows - 1, 0, 1, rows - 1])
    _is(got[torch.from_numpy(k).cuda(), torch.from_numpy(r).cuda()], b.expect["out"](k, r))
    _is(bad, [0, -1])
    assert _lead_intact(whole)


# ---- the excess lists ------------------------------------------------------------------------------------------------------
def test_excess_cols_big_block(ing):
    """t * C + c0 >= 2^32: a time-major block of 1027 channels and 2^32 / 1027 + 6 steps, zeros with values above the
    threshold planted at flat indices 2^32 - 1, 2^32, 2^32 + d and the last one, decoys at the aliases."""
    b, s = _build("excess-cols-big-block")
    T, C, thr, total = s["T"], s["C"], s["threshold"], b.expect["total"]
    whole, body = _led(s["n"], fill=0)
    _plant(body, b.inputs["planted"])
    exc_off, tot = _canary(C + 1, torch.int64), _canary(1, torch.int64)
    scratch = torch.empty(ing.excess_scratch_bytes(ing.EXCESS_COLS, T, C), dtype=torch.uint8, device="cuda")
    ing.excess_count(ing.EXCESS_COLS, body, None, None, None, T, C, thr, exc_off, tot, scratch)
    torch.cuda.synchronize()
    _is(exc_off, b.expect["exc_off"])
    _is(tot, [total])
    pos, val = _canary(total + 8, torch.int32), _canary(total + 8, torch.uint8)
    over = torch.zeros(1, dtype=torch.int64, device="cuda")
    ing.excess_emit(ing.EXCESS_COLS, body, None, None, None, T, C, thr, pos, val, over, scratch)
    torch.cuda.synchronize()
    _is(pos[:total], b.expect["pos"])
    _is(val[:total], b.expect["val"])
    assert bool((pos[total:].contiguous().view(torch.uint8) == bi.CANARY).all()) and bool((val[total:] == bi.CANARY).all())
    _is(over, [0])
    assert total != b.cut["total"] or not np.array_equal(b.expect["val"], b.cut["val"])


# ---- the binner ------------------------------------------------------------------------------------------------------------
def test_bin_long_channel(ing):
    """Bin index and output byte >= 2^32: two channels of 2^32 + 4099 bins, period 3 and a non-zero origin; runs of 1, 2 and
    300 equal ticks in bins 0, 2^32 - 1, 2^32, 2^32 + d and the last one, decoys in bins d and 4098.  The output whole:
    the number of non-zero bytes of each channel, the planted bins, canary around the channels and in the lead."""
    b, s = _build("bin-long-channel")
    T, C, out_off = s["T"], s["C"], s["out_off"]
    whole, out = _led(s["body"])
    ev = types.SimpleNamespace(ticks=torch.from_numpy(b.inputs["ticks"]).cuda(), ev_off=_i64(b.inputs["ev_off"]), C=C)
    d_off = _i64(out_off)
    ing.bin_events(ev, s["origin"], s["period"], T, s["bits"], out, d_off)
    torch.cuda.synchronize()
    for ch in range(C):
        got, bins = out[out_off[ch]:out_off[ch] + T], b.expect["bins"][ch]
        nonzero = sum(int((got[a:a + CHUNK] != 0).sum()) for a in range(0, T, CHUNK))       # (the sum widens its piece)
        assert nonzero == len(bins), (ch, nonzero)
        at = sorted(bins)
        _is(got[_i64(at)], [bins[k] for k in at])
        assert bins != b.cut["bins"][ch]
    assert bool((out[T:out_off[1]] == bi.CANARY).all()) and bool((out[out_off[1] + T:] == bi.CANARY).all())
    assert _lead_intact(whole)


RUNS = {"unbin-far-out": test_unbin_far_out, "unbin-dense-group": test_unbin_dense_group,
        "unbin-csr-long-row": test_unbin_csr_long_row, "unbin-aer-big-block": test_unbin_aer_big_block,
        "aer-far-out": test_aer_far_out, "windows-far-offsets": test_windows_far_offsets,
        "windows-many-items": test_windows_many_items, "excess-cols-big-block": test_excess_cols_big_block,
        "bin-long-channel": test_bin_long_channel}


def test_every_case_of_the_table_is_run():
    assert set(RUNS) == {c.id for c in bi.CASES} and len(bi.CASES) == 9
