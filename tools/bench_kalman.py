"""The Kalman filter decoder (mhk_project, mhk_scan; kalman.KalmanFilter.predict, kalman.cross_validate) against the routes a
user had without it, all in torch on the device.

Same process, the routes alternated after warm-up (20 runs each, fewer where 20 rounds of a group would take more than
--budget seconds: the count stands next to every figure; median and range), device events unless it says host clock.
Results are compared first.
  P  mhk_project, k = 2, at 1024 ch x 1e7 bins and 96 ch x 72 000 bins, against
       matmul   float64 torch.matmul over column chunks (the counts converted chunk by chunk): the only other float64 route.
                Condition: the two routes' run ranges are disjoint, mhk_project's below.
       fir      mhw_fir at one lag, which is float32: reported without a condition.
     and the fraction of the 8 TB/s spec that mhk_project's bytes (rows x cols read, 16 x cols written) make.
  S  mhk_scan at [2, 1e7], one range and five, against the same recurrence in torch at a steady gain: recursive doubling,
     u[t] += F^(2^j) u[t - 2^j], stopped once F^(2^j) is below 2^-60 of its start.  Reported.
  E  predict and cross_validate at 96 x 72 000 against the reference-style loop in torch on the device: one k x k update per
     bin with the gains precomputed (host clock).  Reported.
Prints the table and writes it to --out (default profiles/r22_kalman.txt).

    python tools/bench_kalman.py [--reps 20] [--parts P,S,E] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import muahuff  # noqa: E402
from muahuff import _kalman, _wiener, kalman, wiener  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_events_out import counts_matrix  # noqa: E402
from bench_wiener import alternate, line  # noqa: E402

K = 2
SPEC = 8e12  # bytes per second


def matmul_chunks(x, m, m0, out, chunk):
    for c0 in range(0, x.shape[1], chunk):
        c1 = min(c0 + chunk, x.shape[1])
        torch.addmm(m0.unsqueeze(1), m, x[:, c0:c1].double(), out=out[:, c0:c1])


def part_p(a, lines, res, note):
    met = True
    for rows, T in ((1024, 10 ** 7), (96, 72000)):
        x = counts_matrix(rows, T)
        g = torch.Generator(device="cuda").manual_seed(5)
        m = torch.randn((K, rows), generator=g, device="cuda", dtype=torch.float64) / rows
        m0 = torch.randn((K,), generator=g, device="cuda", dtype=torch.float64)
        v = torch.empty((K, T), dtype=torch.float64, device="cuda")
        want = torch.empty((K, T), dtype=torch.float64, device="cuda")
        w32, b32 = m.float().reshape(K, 1, rows).contiguous(), m0.float().contiguous()
        o32 = torch.empty((K, T), dtype=torch.float32, device="cuda")
        chunk = max(1 << 16, min(T, (1 << 28) // rows))               # the float64 copy of a chunk is at most 2 GiB
        project = lambda: _kalman.project(x.data_ptr(), x.stride(0), rows, T, 255, m, m0, v)  # noqa: E731
        fir = lambda: _wiener.fir(x.data_ptr(), x.stride(0), rows, T, 1, 255, w32, b32, K, o32)  # noqa: E731
        mm = lambda: matmul_chunks(x, m, m0, want, chunk)  # noqa: E731
        project(), mm(), fir()
        scale = float(want.abs().max())
        assert float((v - want).abs().max()) <= 1e-12 * scale and float((o32.double() - want).abs().max()) <= 1e-4 * scale
        say = lambda what: note("P %d x %d: %s" % (rows, T, what))  # noqa: E731
        say("results agree")
        t = alternate([("project", project), ("matmul", mm), ("fir", fir)], a.reps, a.budget, say)
        ok = bool(t["project"]["max"] < t["matmul"]["min"])
        met = met and ok
        byts = rows * T + 8 * K * T
        frac = byts / (t["project"]["median"] * 1e-3) / SPEC
        lines.append("P  %d x %d, k = %d" % (rows, T, K))
        lines.append(line("mhk_project", t["project"]))
        lines.append(line("matmul, float64", t["matmul"]))
        lines.append(line("mhw_fir, 1 lag, f32", t["fir"]))
        lines.append("    matmul / mhk_project x%.2f at the medians; the run ranges %s; %.3g GB in %.4f ms = %.2f of the 8 TB/s spec"
                     % (t["matmul"]["median"] / t["project"]["median"], "are disjoint, mhk_project's below" if ok else "OVERLAP or matmul is faster",
                        byts / 1e9, t["project"]["median"], frac))
        res["P_%dx%d" % (rows, T)] = dict(t, disjoint_and_faster=ok, spec_fraction=round(frac, 4))
        del x, v, want, o32
        torch.cuda.empty_cache()
    return met


def torch_scan(v, F, B, init, ranges, out):
    """the recurrence at one steady gain by recursive doubling"""
    for r, (a, b) in enumerate(ranges):
        out[:, a] = init[r]
        if b - a < 2:
            continue
        u = B @ v[:, a + 1:b]
        u[:, 0] += F @ init[r]
        P, shift, first = F.clone(), 1, float(F.abs().max())
        while shift < b - a - 1 and float(P.abs().max()) > 2.0 ** -60 * first:
            u[:, shift:] += P @ u[:, :-shift]
            P, shift = P @ P, 2 * shift
        out[:, a + 1:b] = u
    return out


def part_s(a, lines, res, note):
    T = 10 ** 7
    g = torch.Generator(device="cuda").manual_seed(6)
    v = torch.randn((K, T), generator=g, device="cuda", dtype=torch.float64)
    th = 0.15
    F = 0.9 * torch.tensor([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]], dtype=torch.float64, device="cuda")
    B = torch.randn((K, K), generator=g, device="cuda", dtype=torch.float64)
    out, want = torch.empty_like(v), torch.empty_like(v)
    for n in (1, 5):
        ranges = [(i * (T // n), (i + 1) * (T // n)) for i in range(n)]
        init = torch.randn((n, K), generator=g, device="cuda", dtype=torch.float64)
        scratch = torch.empty((_kalman.scan_scratch_bytes(T, K, n),), dtype=torch.uint8, device="cuda")
        scan = lambda: _kalman.scan(v, ranges, F.unsqueeze(0), B.unsqueeze(0), init, out, scratch)  # noqa: E731
        doubling = lambda: torch_scan(v, F, B, init, ranges, want)  # noqa: E731
        scan(), doubling()
        assert float((out - want).abs().max()) <= 1e-11 * float(want.abs().max())
        say = lambda what: note("S %d range(s): %s" % (n, what))  # noqa: E731
        say("results agree")
        t = alternate([("scan", scan), ("doubling", doubling)], a.reps, a.budget, say)
        byts = 3 * 8 * K * T                                          # v read twice, out written once
        lines.append("S  [%d, %d], %d range%s" % (K, T, n, "" if n == 1 else "s"))
        lines.append(line("mhk_scan", t["scan"]))
        lines.append(line("torch, doubling", t["doubling"]))
        lines.append("    doubling / mhk_scan x%.2f at the medians; %.3g GB in %.4f ms = %.2f of the 8 TB/s spec"
                     % (t["doubling"]["median"] / t["scan"]["median"], byts / 1e9, t["scan"]["median"], byts / (t["scan"]["median"] * 1e-3) / SPEC))
        res["S_%d" % n] = t


def loop_predict(f, x, y0, ranges, Fd, Bd):
    """the reference's loop on the device: z-score, then one update per bin with the tabulated gains"""
    n_gain = Fd.shape[0]
    v = f.m @ torch.clamp(x, max=f.clip).double() + f.m0.unsqueeze(1)
    out = torch.full_like(v, float("nan"))
    for r, (a, b) in enumerate(ranges):
        s = y0[r] - f.mean_y
        out[:, a] = s
        for t in range(a + 1, b):
            i = min(t - a - 1, n_gain - 1)
            s = Fd[i] @ s + Bd[i] @ v[:, t]
            out[:, t] = s
    return out + f.mean_y.unsqueeze(1)


def loop_cross_validate(x, y, lead, alphas, num_fold):
    fr = wiener.fold_ranges(x.shape[1] - lead, num_fold)
    st = kalman.stats(x, y, lead, None, fr)
    res = torch.empty((len(alphas), num_fold, 2, K), dtype=torch.float64, device=x.device)
    for i in range(num_fold):
        v, t = i, (i + 1) % num_fold
        tot = sum(st[k] for k in range(num_fold) if k not in (v, t))
        for j, al in enumerate(alphas):
            f = kalman.KalmanFilter(al).fit(tot)
            Fd, Bd = f._device_table(x.device)
            hs = sorted((fr[v], fr[t]))
            y0 = torch.stack([y[:, c + lead] for c, _d in hs]).double()
            pred = loop_predict(f, x, y0, hs, Fd, Bd)
            for h, (c, d) in enumerate((fr[v], fr[t])):
                res[j, i, h] = torch.sqrt(((pred[:, c:d] - y[:, c + lead:d + lead].double()) ** 2).mean(1))
    return res


def host_clock(fns, reps, note):
    ts = {k: [] for k, _ in fns}
    for i in range(reps):
        for k, f in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
        note("round %d of %d" % (i + 1, reps))
    return {k: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4), runs=len(v)) for k, v in ts.items()}


def part_e(a, lines, res, note):
    rows, T, lead, folds, alphas = 96, 72000, 2, 5, (0.0, 1e-2)
    sys.path.insert(0, ROOT)
    from tests import kalman_oracle as ko
    xh, yh = ko.data(rows, K, T, 3)
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
    f = kalman.KalmanFilter(0.0).fit(kalman.stats(x, y, lead))
    Fd, Bd = f._device_table(x.device)
    rs = [(0, T - lead)]
    y0 = y[:, lead:lead + 1].t().double()
    got, want = f.predict(x, y0, rs), loop_predict(f, x, y0, rs, Fd, Bd)
    assert float((got - want)[:, :T - lead].abs().max()) <= 1e-10 * float(want[:, :T - lead].abs().max())
    say = lambda what: note("E: %s" % what)  # noqa: E731
    say("predictions agree; the gain table has %d entries" % Fd.shape[0])
    reps = max(3, min(a.reps, 5))
    t = host_clock([("predict", lambda: f.predict(x, y0, rs)), ("loop", lambda: loop_predict(f, x, y0, rs, Fd, Bd))], reps, say)
    lines.append("E  %d x %d, k = %d, lead %d (host clock)" % (rows, T, K, lead))
    lines.append(line("predict", t["predict"]))
    lines.append(line("torch loop per bin", t["loop"]))
    lines.append("    loop / predict x%.0f at the medians" % (t["loop"]["median"] / t["predict"]["median"]))
    res["E_predict"] = t
    cv = kalman.cross_validate(x, y, lead, None, alphas, folds)
    hand = loop_cross_validate(x, y, lead, alphas, folds)
    assert torch.allclose(cv["rmse_valid"], hand[:, :, 0], rtol=1e-8, atol=0) and torch.allclose(cv["rmse_test"], hand[:, :, 1], rtol=1e-8, atol=0)
    say("cross-validation agrees")
    t = host_clock([("cross_validate", lambda: kalman.cross_validate(x, y, lead, None, alphas, folds)),
                    ("loop", lambda: loop_cross_validate(x, y, lead, alphas, folds))], 3, say)
    lines.append("E  cross_validate, %d folds, alphas %s (host clock)" % (folds, alphas))
    lines.append(line("cross_validate", t["cross_validate"]))
    lines.append(line("torch loop per bin", t["loop"]))
    lines.append("    loop / cross_validate x%.0f at the medians" % (t["loop"]["median"] / t["cross_validate"]["median"]))
    res["E_cross_validate"] = t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="P,S,E")
    ap.add_argument("--budget", type=float, default=40.0, help="seconds of timed rounds per group of alternated routes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_kalman.txt"))
    a = ap.parse_args()
    info = muahuff.device_info(0)
    lines = ["bench_kalman: %s (%s), %d alternated runs" % (info["name"], info["arch"], a.reps)]
    res, met = {}, True
    note = lambda what: print(what, file=sys.stderr, flush=True)  # noqa: E731
    parts = a.parts.split(",")
    if "P" in parts:
        met = part_p(a, lines, res, note) and met
    if "S" in parts:
        part_s(a, lines, res, note)
    if "E" in parts:
        part_e(a, lines, res, note)
    lines.append("condition (mhk_project below float64 matmul, run ranges disjoint, both shapes): %s" % ("met" if met else "NOT met"))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
