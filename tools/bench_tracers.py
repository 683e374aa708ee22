"""Added time per step of the device-side tracers (cfd_tracers_*): two models
of the same grid step side by side, one with tracers enabled, in interleaved
cfd_timing_begin/end windows of K steps, R times; tracers only read the flow,
so both models do the same solver work.  Prints one JSON line per case with
the medians, the spread of each side and the difference.

Cases: `channel` -- the default 800 x 264 channel, tracers injected every 100
steps over DEVELOP steps (a developed population); `cavity` -- the 4096^2
cavity of bench.py, seeded through cfd_tracers_set with N tracers.

Usage: python tools/bench_tracers.py [channel|cavity ...] [--k K] [--r R] [--n N] [--develop D]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo_amd"))
import cfdamd  # noqa: E402


def window(m, k):
    m.timing_begin()
    m.update_n(k)
    t = m.timing_end()
    return t["step_ms"] / t["steps"] * 1e3   # us per step


def run(name, grid, params, develop, seed_n, k, r):
    plain, traced = cfdamd.Model(grid, params), cfdamd.Model(grid, params)
    try:
        if seed_n:
            plain.update_n(develop)
            traced.update_n(develop)
            traced.tracers_enable(seed_n + grid.ny, 1 << 30)   # no injection while timing
            rng = np.random.default_rng(1)
            traced.set_tracers(rng.uniform(0.02, 0.98, seed_n) * grid.lx,
                               rng.uniform(0.02, 0.98, seed_n) * grid.ly, np.zeros(seed_n))
        else:
            traced.tracers_enable(1 << 16, 100)
            plain.update_n(develop)
            traced.update_n(develop)
        n0 = traced.tracer_count()
        window(plain, k), window(traced, k)   # warm both paths
        a, b = [], []
        for _ in range(r):
            a.append(window(plain, k))
            b.append(window(traced, k))
        n1 = traced.tracer_count()
        ma, mb = statistics.median(a), statistics.median(b)
        added = mb - ma
        n = 0.5 * (n0 + n1)
        print(json.dumps({
            "case": name, "nx": grid.nx, "ny": grid.ny, "k": k, "r": r,
            "tracers_before": n0, "tracers_after": n1,
            "us_per_step_disabled": [round(x, 2) for x in a],
            "us_per_step_enabled": [round(x, 2) for x in b],
            "median_disabled": round(ma, 2), "median_enabled": round(mb, 2),
            "spread_disabled": round(max(a) - min(a), 2), "spread_enabled": round(max(b) - min(b), 2),
            "added_us_per_step": round(added, 2),
            "tracers_per_s": round(n / (added * 1e-6)) if added > 0 else None,
            # 48 B of state read and 48 B written per tracer, moved in place and compacted:
            # x, y read + written by the advect launch, x, y, initialY read + written by the scatter
            "state_GB_per_s": round(n * 80 / (added * 1e-6) / 1e9, 1) if added > 0 else None,
        }), flush=True)
    finally:
        plain.close()
        traced.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["channel", "cavity"])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--r", type=int, default=7)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--develop", type=int, default=0)
    args = ap.parse_args()
    for case in args.cases:
        if case == "channel":
            run(case, cfdamd.default_grid(), cfdamd.SimulationParams(), args.develop or 1500, 0,
                args.k, args.r)
        elif case == "cavity":
            run(case, cfdamd.cavity_grid(4096),
                cfdamd.SimulationParams.cavity(1000.0, 200, corrector_passes=0, tol_enabled=False),
                args.develop or 100, args.n, args.k, args.r)
        else:
            raise SystemExit(f"unknown case {case}")


if __name__ == "__main__":
    main()
