#!/usr/bin/env python
"""Rate of the spin-polarization launch (mode 5, is3d_launch_polarization) on one GPU, with the same build's Grad
k_spectra launch at the same shape as the yardstick.

Shape: 10^5 cells 3+1D x [3122, -3122, 3312, 3334] x pT48 x phi32 x y21 (tests/test_gpu_polzn.py's realistic
size).  Both launches are timed with device events on one stream around `steps` back-to-back launches after
`warmup` untimed ones; the output stays resident.  Prints one JSON line:

  polzn_ms, polzn_points_per_s        cell x species x momentum points / s of is3d_launch_polarization
  spectra_grad_ms, spectra_grad_points_per_s   the same for is3d_launch (df_mode 1, both delta-f corrections on)
  build_id                            is3d_build_id() of the library measured

    python tools/polzn_bench.py [--cells 100000] [--steps 30] [--warmup 5] [--repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, launch, finish, steps, warmup, repeats):
    for _ in range(warmup):
        launch()
    finish()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            launch()
        t1.record()
        finish()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / steps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("polzn_bench needs a GPU")
    torch.cuda.init()
    from is3d2_amd import _lib, build_engine, make_spec, synth

    n = a.cells
    chosen = [3122, -3122, 3312, 3334]
    spec = make_spec(chosen=chosen, pT="pT48", phi="phi32", y="y21", dimension=3, df_mode=1)
    surf = synth.as_read(synth.surface(n, seed=77, dimension=3, full3d=True))
    w = synth.vorticity(n, 5)
    e = build_engine(spec, dict(surf, **{k: w[i] for i, k in enumerate(_lib.VORTICITY_FIELDS)}), device=0)
    size = e.output_size()
    sp = spec["species"]
    classes = len(set(zip(np.asarray(sp["mass"]).tolist(), np.asarray(sp["sign"]).tolist())))   # by (mass, sign)
    points = float(n) * len(chosen) * len(spec["pT"]) * len(spec["phi"]) * len(spec["y"])
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(5 * size, dtype=torch.float64, device="cuda:0")
    T_avg = 0.150

    pol = timed(torch, lambda: e.launch_polarization(T_avg, out.data_ptr(), stream), e.finish, a.steps, a.warmup, a.repeats)
    pol_splits = e.get_tuning("splits")
    spe = timed(torch, lambda: e.launch(out.data_ptr(), stream), e.finish, a.steps, a.warmup, a.repeats)
    res = dict(tool="polzn_bench", cells=n, species=len(chosen), classes=classes, npT=len(spec["pT"]), nphi=len(spec["phi"]),
               ny=len(spec["y"]), steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               polzn_ms=min(pol), polzn_ms_all=pol, polzn_points_per_s=points / (min(pol) * 1e-3), polzn_splits=pol_splits,
               spectra_grad_ms=min(spe), spectra_grad_ms_all=spe, spectra_grad_points_per_s=points / (min(spe) * 1e-3),
               build_id=_lib.build_id(), device=torch.cuda.get_device_name(0))
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
