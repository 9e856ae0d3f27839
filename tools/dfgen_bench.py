#!/usr/bin/env python
"""Time of the delta-f coefficient generator (is3d_generate_df_tables, dfgen.hip) on one GPU, next to the host build of
the same math (is3d2_amd/csrc/dfgen_math.h through tests/native/dfgen_emulator.cpp, OpenMP) on the same grid.

Shape: the shipped 101 x 81 (T, muB) grid for the three shipped hadron lists (UrQMD, SMASH, SMASH box), 64-point
Gauss-Laguerre table.  `warmup` untimed calls, then `repeats` timed ones; the time is the host clock around the whole
call (uploads, the launch, the download of the ten tables).  One JSON line per list:

  ms / ms_min / ms_max / ms_all   median, range and every repeat of the call
  hadrons, points                 list rows (antibaryons included) and grid points
  node_evals_per_s                points x hadrons x 4 families x 64 nodes / s (an upper count: family 1 and the
                                  baryon-only sums skip the mesons)
  max_abs_vs_shipped              largest |value - shipped value| over the ten tables (the files hold six decimals)
  cpu_ms, cpu_threads             the emulator on the same grid with OMP_NUM_THREADS threads (default 16), one run
  build_id                        is3d_build_id() of the library measured

    python tools/dfgen_bench.py [--repeats 5] [--warmup 1] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from is3d2_amd import Engine, _lib, hrg
    from is3d2_amd import data as D
    for h, name in ((1, "urqmd"), (2, "smash"), (3, "smash_box")):
        parts = hrg.pdg_particles(h)
        T, muB, shipped = D.df_tables(h)
        e = Engine()
        e.set_pdg(parts["mass"], parts["sign"], parts["gspin"], parts["baryon"])
        e.set_gauss_laguerre(*D.gauss_laguerre(64))
        ms = []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            tab = e.generate_df_tables(T, muB)
            w = 1e3 * (time.perf_counter() - t0)
            if r >= a.warmup:
                ms.append(w)
        e.close()
        nh, npt = len(parts["mass"]), len(T) * len(muB)
        t = float(np.median(ms))
        out = dict(list=name, hadrons=nh, grid=[len(T), len(muB)], points=npt, ms=round(t, 3), ms_min=round(min(ms), 3),
                   ms_max=round(max(ms), 3), ms_all=[round(v, 3) for v in ms],
                   node_evals_per_s=npt * nh * 4 * 64 / (t * 1e-3), max_abs_vs_shipped=float(np.max(np.abs(tab - shipped))),
                   build_id=_lib.build_id())
        if not a.no_cpu:
            import df_gen_ref as R
            R.emulator()        # built outside the timed window
            t0 = time.perf_counter()
            emu, _ = R.emulate(parts, T, muB)
            out.update(cpu_ms=round(1e3 * (time.perf_counter() - t0), 3), cpu_threads=int(os.environ["OMP_NUM_THREADS"]),
                       max_excess_vs_cpu=float(np.max(R.ref_excess(tab, emu))))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
