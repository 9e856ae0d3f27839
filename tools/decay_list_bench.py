#!/usr/bin/env python
"""Time of the Monte Carlo resonance decays of a sampled list (is3d_decay_sampled, decay_list.hip) on one GPU, next to
the host build of the same math (is3d2_amd/csrc/decay_mc_math.h in tests/native/decay_list_emulator.cpp, OpenMP).

Shape: the SMASH decay table (tests/golden/decays_smash.npz, 444 chosen species) and a list of about --primaries
(default 10^6) thermal hadrons sampled from a synthetic 2+1D surface of --cells cells (df_mode 2); the number of events
is chosen from a two-event trial.  Every repeat samples the list again (outside the timed window: is3d_decay_sampled
replaces the engine's list) and then calls is3d_decay_sampled with bin = 0 and nothing else.  `warmup` untimed calls,
then `repeats` timed ones.  One JSON line:

  ms / ms_range / ms_all      device time of one call between the HIP events of its batches (decay_list_stats ms_total):
                              median, [min, max], every repeat
  wall_ms                     median host time around the call: upload of the primaries, kernels, download of the list
  transfer_share              (wall_ms - ms) / wall_ms: the share of upload, download and host bookkeeping
  decays_per_s                decays / device time; decays_per_s_wall: / host time
  primaries, decays, final_particles, passes, batches
  cpu_ms, cpu_decays_per_s    the emulator on the same list with OMP_NUM_THREADS threads (default 16), the whole host
                              call (table build, trees, copy out); cpu_equal: its list has the GPU's species and origins
  build_id                    is3d_build_id() of the library measured

--four-body: the UrQMD rows of tests/golden/decays_urqmd_subset.npz over the UrQMD chosen list through
is3d_set_decays4 (nine four-body rows: f2(1270), f1(1285), f0(1370)), and in addition
  four_body_decays, four_body_share   decays through a four-body channel (primaries of their parents x the channels'
                              branching: nothing in the subset feeds those parents), and their share of all decays
  four_body_tries             mean tries of the four-body rejection loop, 1 / acceptance of the engine's own draw
                              (10^6 tries per parent mass on the host), weighted by those decays

    python tools/decay_list_bench.py [--repeats 5] [--warmup 1] [--primaries 1000000] [--cells 1000] [--no-cpu] [--four-body]
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
    ap.add_argument("--primaries", type=int, default=1_000_000)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--four-body", action="store_true")
    a = ap.parse_args()
    from is3d2_amd import _lib, build_engine, hrg, make_spec, surface_averages, synth
    if a.four_body:
        d = dict(np.load(os.path.join(ROOT, "tests", "golden", "decays_urqmd_subset.npz")))
        spec = make_spec(hrg_eos=1, chosen="urqmd", df_mode=2, dimension=2)
    else:
        d = dict(np.load(os.path.join(ROOT, "tests", "golden", "decays_smash.npz")))
        spec = make_spec(hrg_eos=2, chosen="smash", df_mode=2, dimension=2)
    mcids = spec["species"]["mcid"]
    ch = hrg.decay_channels(d, d, mcids, four_body=a.four_body)
    s = synth.as_read(synth.surface(a.cells, seed=a.seed))
    plasma = surface_averages(s, 0)
    e = build_engine(spec, s, T_avg=plasma[0])
    e.set_decays(ch)
    trial, _, _ = e.sample(a.seed, 2, 0.5, 0, plasma)
    nev = max(1, int(round(a.primaries / max(len(trial) / 2.0, 1.0))))
    ms, wall = [], []
    for r in range(a.warmup + a.repeats):
        prim, off0, _ = e.sample(a.seed, nev, 0.5, 0, plasma)
        t0 = time.perf_counter()
        rc = e.lib.is3d_decay_sampled(e._e, a.seed, 0)
        w = 1e3 * (time.perf_counter() - t0)
        if rc:
            raise RuntimeError(e.lib.is3d_last_error(e._e).decode())
        if r >= a.warmup:
            ms.append(e.decay_list_stats()["ms_total"])
            wall.append(w)
    st = e.decay_list_stats()
    out_parts, origins = e._decayed_list()
    t, tw = float(np.median(ms)), float(np.median(wall))
    out = dict(species=len(mcids), channels=len(ch), kept=e.decay_stats()["kept"], cells=a.cells, events=nev,
               primaries=st["primaries"], decays=st["decays"], undecayed=st["undecayed"], dropped_daughters=st["dropped_daughters"],
               capped=st["capped"], final_particles=st["final_particles"], passes=st["passes"], batches=st["batches"],
               ms=round(t, 3), ms_range=[round(min(ms), 3), round(max(ms), 3)], ms_all=[round(v, 3) for v in ms],
               wall_ms=round(tw, 3), transfer_share=round((tw - t) / tw, 3), decays_per_s=st["decays"] / (t * 1e-3),
               decays_per_s_wall=st["decays"] / (tw * 1e-3), build_id=_lib.build_id())
    e.close()
    if a.four_body:
        import decay4_ref as D4
        four = ch[ch["n_body"] == 4]
        counts = np.bincount(prim["species"], minlength=len(mcids))
        n4 = tries = 0.0
        for p in sorted(set(four["parent"].tolist())):
            rows = four[four["parent"] == p]
            k = counts[p] * rows["branching"].sum()
            n4 += k
            tries += k / D4.envelope(rows["mass_parent"][0], rows["mass"][0], a.seed, 1_000_000)[1]
        out.update(four_body_channels=len(four), four_body_decays=round(n4), four_body_share=n4 / max(st["decays"], 1),
                   four_body_tries=tries / max(n4, 1.0))
    if not a.no_cpu:
        import decay_list_ref as L
        emulator, emulate = (D4.emulator, D4.emulate_list) if a.four_body else (L.emulator, L.emulate)
        emulator()          # built outside the timed window
        t0 = time.perf_counter()
        ref, _, orig_r, cst, _ = emulate(spec["species"]["mass"], ch, prim, off0, a.seed)
        ct = time.perf_counter() - t0
        out.update(cpu_threads=int(os.environ["OMP_NUM_THREADS"]), cpu_ms=round(ct * 1e3, 3), cpu_decays_per_s=cst["decays"] / ct,
                   cpu_equal=bool(len(ref) == len(out_parts) and np.array_equal(ref["species"], out_parts["species"]) and
                                  np.array_equal(orig_r, origins)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
