#!/usr/bin/env python
"""Time of operation = 0 (spacetime distributions dN/dX) for the modified-momentum modes on one GPU, in one process:
PTM and PTB through Engine.calculate_dN_dX, PTMA (df_mode 5) through Engine.calculate_dN_dX_famod with
famod_chains = 1.  bench.py times the flagship workload and calls calculate_dN_dX for operation 0, which has no
df_mode 5 path; this tool is the rate of the PTMA entry next to the two modes whose lane forms it shares.

Shape: 10^5 synth 3+1D cells (full3d), the SMASH species, pT48 x phi32 x y21.  Each mode runs `warmup` untimed calls
and `repeats` timed ones.  One JSON line per mode:

  ms, ms_range            median host wall time of one call and the repeats' (min, max)
  ms_prepass, ms_kernel   the stats' device times of the median call's stages: the prepass (PTMA: with the Newton
                          solves along the chain, which every call runs again) and the k_dndx launches
  ms_device               the stats' device time of the whole call
  breakdown, iterations   PTMA: the prepass counters
  spectra_ms_prepass, spectra_ms_kernel, spectra_iterations
                          PTMA: the same engine's calculate_spectra (operation 1) on the same surface, whose prepass
                          solves the same chain (tools/ptma_chain_probe.py's figure for this surface)
  build_id                is3d_build_id() of the library measured

--existing-only leaves the PTMA row out: the PTM / PTB rows then run on a library without the new entry.

    python tools/dndx_famod_bench.py [--cells 100000] [--repeats 3] [--warmup 1] [--existing-only]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--existing-only", action="store_true")
    a = ap.parse_args()
    from is3d2_amd import _lib, build_engine, make_spec, surface_averages, synth
    s = synth.as_read(synth.surface(a.cells, seed=7, dimension=3, full3d=True))
    T_avg = surface_averages(s, 0)[0]
    for mode in ((3, 4) if a.existing_only else (3, 4, 5)):
        spec = make_spec(hrg_eos=2, chosen="smash", df_mode=mode, dimension=3, pT="pT48", phi="phi32", y="y21",
                         famod_chains=1)
        e = build_engine(spec, s, T_avg=T_avg)
        call = e.calculate_dN_dX_famod if mode == 5 else e.calculate_dN_dX
        for _ in range(a.warmup):
            call()
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            runs.append((1e3 * (time.perf_counter() - t0), e.stats()))
        runs.sort(key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        out = dict(df_mode=mode, entry=call.__name__, cells=a.cells, species=len(spec["species"]["mass"]),
                   grid=[len(spec["pT"]), len(spec["phi"]), len(spec["y"])], ms=round(ms, 3),
                   ms_range=[round(runs[0][0], 3), round(runs[-1][0], 3)], ms_prepass=round(st["ms_prepass"], 3),
                   ms_kernel=round(st["ms_spectra"], 3), ms_device=round(st["ms_total"], 3),
                   ms_kernel_range=[round(min(r[1]["ms_spectra"] for r in runs), 3), round(max(r[1]["ms_spectra"] for r in runs), 3)],
                   build_id=_lib.build_id())
        if mode == 5:
            out.update(famod_chains=1, breakdown=st["breakdown"], iterations=st["iterations"])
            # the comparison point of the prepass: the same engine's operation 1, which solves the same chain
            e.calculate_spectra()
            e.calculate_spectra()
            sp = e.stats()
            out.update(spectra_ms_prepass=round(sp["ms_prepass"], 3), spectra_ms_kernel=round(sp["ms_spectra"], 3),
                       spectra_iterations=sp["iterations"])
        print(json.dumps(out), flush=True)
        e.close()


if __name__ == "__main__":
    main()
