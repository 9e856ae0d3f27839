#!/usr/bin/env python
"""Rate of the particle sampler (operation = 2, is3d_sample) on one GPU, next to the serial CPU emulator of the same
math (tests/native/sampler_emulator.cpp) on a prefix of the cells.

Shape: BASELINE config-2-like -- 10^5 3+1D cells (synth, full3d), SMASH species, Grad and PTB, fast = 0 and 1, a few
events.  Each configuration is sampled `warmup` untimed times and `repeats` timed ones; the time is the host wall
time of Engine.sample: the cell prologue, every batch's kernels and scans, and the copy of the list to the host.
There is no reference figure: the reference sampler needs GSL.  Prints one JSON line per configuration:

  ms                       median wall time of one is3d_sample call
  candidates_per_s         Poisson candidates / s
  accepted_per_s           kept hadrons / s
  efficiency               momentum rejection loop: acceptances / proposals
  cpu_candidates_per_s     the serial emulator on the first --cpu-cells cells, one core
  build_id                 is3d_build_id() of the library measured

--binned: after the list call, and in the same process, the same protocol times Engine.sample_binned(keep_list=False)
-- the test_sampler = 1 form that bins every kept particle on the device (the reference's default bins) and builds no
list -- and adds binned_ms, binned_ms_all, binned_batches, binned_candidates_per_s, binned_accepted_per_s; the counts of
the two calls must agree.

--famod: one more row, df_mode 5 through Engine.sample_famod (and sample_famod_binned with --binned), famod_chains = 1:
the time includes the Newton prepass along the chain, which every call runs again (its share is read from a kernel
trace, not from this tool); famod_stats are the reconstruction counters.  There is no fast branch and no CPU column.

    python tools/sampler_bench.py [--cells 100000] [--events 8] [--repeats 3] [--warmup 1] [--cpu-cells 2000] [--binned]
                                  [--famod] [--famod-only]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--events", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-cells", type=int, default=2000)
    ap.add_argument("--binned", action="store_true")
    ap.add_argument("--famod", action="store_true")
    ap.add_argument("--famod-only", action="store_true")
    a = ap.parse_args()
    from is3d2_amd import _lib, build_engine, make_spec, surface_averages, synth
    s = synth.as_read(synth.surface(a.cells, seed=7, dimension=3, full3d=True))
    plasma = surface_averages(s, 0)
    for mode in (() if a.famod_only else (1, 4)):
        spec = make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=3)
        e = build_engine(spec, s, T_avg=plasma[0])
        if a.binned:
            e.set_sample_bins()
        for fast in (0, 1):
            for _ in range(a.warmup):
                e.sample(1, a.events, 0.5, fast, plasma)
            ms = []
            for r in range(a.repeats):
                t0 = time.perf_counter()
                p, off, st = e.sample(1, a.events, 0.5, fast, plasma)
                ms.append(1e3 * (time.perf_counter() - t0))
            t = float(np.median(ms)) * 1e-3
            out = dict(df_mode=mode, fast=fast, cells=a.cells, events=a.events, species=len(spec["species"]["mass"]),
                       ms=round(t * 1e3, 3), ms_all=[round(v, 3) for v in ms], candidates=st["candidates"],
                       kept=st["kept"], candidates_per_s=st["candidates"] / t, accepted_per_s=st["kept"] / t,
                       efficiency=st["acceptances"] / max(st["proposals"], 1), capped=st["capped"],
                       batches=st["batches"], build_id=_lib.build_id())
            if a.binned:
                for _ in range(a.warmup):
                    e.sample_binned(1, a.events, 0.5, fast, plasma)
                bms = []
                for r in range(a.repeats):
                    t0 = time.perf_counter()
                    hist, bst = e.sample_binned(1, a.events, 0.5, fast, plasma)
                    bms.append(1e3 * (time.perf_counter() - t0))
                assert bst["kept"] == st["kept"] and bst["candidates"] == st["candidates"]
                assert int(hist["dN_dphipdy"].sum()) == st["kept"]
                bt = float(np.median(bms)) * 1e-3
                out.update(binned_ms=round(bt * 1e3, 3), binned_ms_all=[round(v, 3) for v in bms], binned_batches=bst["batches"],
                           binned_candidates_per_s=bst["candidates"] / bt, binned_accepted_per_s=bst["kept"] / bt)
            if a.cpu_cells > 0:
                import sampler_ref as R
                t0 = time.perf_counter()
                _, cst, _ = R.sample(spec, s, plasma, 1, a.events, 0.5, fast, 0, min(a.cpu_cells, a.cells))
                ct = time.perf_counter() - t0
                out.update(cpu_cells=min(a.cpu_cells, a.cells), cpu_ms=round(ct * 1e3, 3),
                           cpu_candidates_per_s=cst["candidates"] / ct)
            print(json.dumps(out), flush=True)
        e.close()
    if a.famod or a.famod_only:
        spec = make_spec(hrg_eos=2, chosen="smash", df_mode=5, dimension=3)
        e = build_engine(spec, s, T_avg=plasma[0])

        def timed(call):
            for _ in range(a.warmup):
                call()
            ms = []
            for r in range(a.repeats):
                t0 = time.perf_counter()
                res = call()
                ms.append(1e3 * (time.perf_counter() - t0))
            return res, ms, float(np.median(ms)) * 1e-3
        (p, off, st), ms, t = timed(lambda: e.sample_famod(1, a.events, 0.5))
        out = dict(df_mode=5, famod_chains=1, cells=a.cells, events=a.events, species=len(spec["species"]["mass"]),
                   ms=round(t * 1e3, 3), ms_all=[round(v, 3) for v in ms], candidates=st["candidates"], kept=st["kept"],
                   candidates_per_s=st["candidates"] / t, accepted_per_s=st["kept"] / t,
                   efficiency=st["acceptances"] / max(st["proposals"], 1), capped=st["capped"], batches=st["batches"],
                   breakdown=st["breakdown"], famod_stats=e.sample_famod_stats(), build_id=_lib.build_id())
        if a.binned:
            e.set_sample_bins()
            (hist, bst), bms, bt = timed(lambda: e.sample_famod_binned(1, a.events, 0.5))
            assert bst["kept"] == st["kept"] and bst["candidates"] == st["candidates"]
            out.update(binned_ms=round(bt * 1e3, 3), binned_ms_all=[round(v, 3) for v in bms], binned_batches=bst["batches"],
                       binned_candidates_per_s=bst["candidates"] / bt, binned_accepted_per_s=bst["kept"] / bt)
        print(json.dumps(out), flush=True)
        e.close()


if __name__ == "__main__":
    main()
