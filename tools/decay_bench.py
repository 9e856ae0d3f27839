#!/usr/bin/env python
"""Time of the resonance-decay feed-down (is3d_launch_feeddown, decay.hip) on one GPU, next to the CPU emulator of the
same math (tests/native/decay_emulator.cpp, OpenMP) on a prefix of the channels.

Shape: the SMASH decay table (tests/golden/decays_smash.npz, 444 chosen species) on the BASELINE momentum grid,
48 pT x 32 phi x 21 y in 3+1D and 48 x 32 x 1 in 2+1D.  The spectra are thermal, exp(-mT / T)(1 + 2 v2 cos 2 phi)
exp(-y^2 / 8): the feed-down's work does not depend on the values (apart from the rare non-positive entries).  The
spectra stay resident on the device; every call starts from the same thermal spectra (a device copy outside the timed
window).  `warmup` untimed calls, then `repeats` timed ones; the time is the device time between the two HIP events of
is3d_launch_feeddown (decay_stats ms_total), and next to it the host clock around launch + finish.  One JSON line each:

  ms / ms_all / wall_ms       median device time of one call, every repeat, median host time
  slots, terms                daughter slots that receive feed-down; two-body terms (a 3-body slot has 12)
  points                      pT x phi x y
  node_evals_per_s            terms x points x 144 (v, zeta) nodes / s; each evaluates the parent at two angles
  cpu_*                       the emulator on the first --cpu-channels channels with OMP_NUM_THREADS threads (default 16)
  build_id                    is3d_build_id() of the library measured

--four-body: the UrQMD rows of tests/golden/decays_urqmd_subset.npz over the UrQMD chosen list, once through
is3d_set_decays (the nine four-body rows skipped) and once through is3d_set_decays4: the second line's added_terms is
the number of two-body terms the four-body slots add (12 each); no CPU run.

    python tools/decay_bench.py [--repeats 5] [--warmup 1] [--cpu-channels 60] [--dims 3,2] [--four-body]
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


def work(ch, stats):
    """(slots, terms) of a channel table none of whose channels is skipped as closed."""
    assert stats["skipped_closed"] == 0
    sel = (ch["n_body"] == 2) | (ch["n_body"] == 3) | ((ch["n_body"] == 4) & (stats["skipped_many_body"] == 0))
    per = np.array([(c["daughter"][:c["n_body"]] >= 0).sum() for c in ch[sel]])
    return int(per.sum()), int((per * np.where(ch["n_body"][sel] >= 3, 12, 1)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-channels", type=int, default=60)
    ap.add_argument("--dims", default="3,2")
    ap.add_argument("--four-body", action="store_true")
    a = ap.parse_args()
    import torch
    from is3d2_amd import Engine, _lib, hrg
    from is3d2_amd import data as D
    name, eos = ("urqmd_subset", 1) if a.four_body else ("smash", 2)
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "decays_%s.npz" % name)))
    parts = hrg.pdg_particles(eos)
    mcids = hrg.chosen_mcids("urqmd" if a.four_body else "smash")
    sp = hrg.chosen_species(parts, mcids)
    (pT, _), (phi, _), (y21, _) = D.grid("pT48"), D.grid("phi32"), D.grid("y21")
    runs = [(dim, four) for dim in [int(v) for v in a.dims.split(",")] for four in ((False, True) if a.four_body else (False,))]
    base_terms = {}
    for dim, four in runs:
        ch = hrg.decay_channels(d, d, mcids, four_body=four)
        y = y21 if dim == 3 else np.zeros(1)
        S = np.exp(-np.sqrt(pT[None, :, None, None] ** 2 + sp["mass"][:, None, None, None] ** 2) / 0.15) * \
            (1 + 0.1 * np.cos(2 * phi))[None, None, :, None] * np.exp(-y ** 2 / 8)[None, None, None, :]
        e = Engine()
        e.set_params(dimension=dim)
        e.set_species(sp["mass"], sp["sign"], sp["degen"], sp["baryon"])
        e.set_momentum_grid(pT, phi, y, np.zeros(1), np.ones(1))
        e.set_decays(ch)
        thermal = torch.from_numpy(np.ascontiguousarray(S)).to("cuda:0")
        buf = torch.empty_like(thermal)
        stream = torch.cuda.current_stream(0).cuda_stream
        ms, wall = [], []
        for r in range(a.warmup + a.repeats):
            buf.copy_(thermal)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.launch_feeddown(buf.data_ptr(), stream)
            e.finish()
            w = 1e3 * (time.perf_counter() - t0)
            if r >= a.warmup:
                ms.append(e.decay_stats()["ms_total"])
                wall.append(w)
        st = e.decay_stats()
        slots, terms = work(ch, st)
        points = len(pT) * len(phi) * len(y)
        t = float(np.median(ms)) * 1e-3
        out = dict(dimension=dim, species=len(mcids), grid=[len(pT), len(phi), len(y)], channels=len(ch), kept=st["kept"],
                   adjusted=st["adjusted"], levels=st["levels"], slots=slots, terms=terms, points=points,
                   ms=round(t * 1e3, 3), ms_all=[round(v, 3) for v in ms], wall_ms=round(float(np.median(wall)), 3),
                   node_evals_per_s=terms * points * 144 / t, build_id=_lib.build_id())
        if a.four_body:
            base_terms.setdefault(dim, terms)
            out.update(four_body=four, skipped_many_body=st["skipped_many_body"], added_terms=terms - base_terms[dim])
        got = buf.cpu().numpy()
        e.close()
        if a.cpu_channels > 0 and not a.four_body:
            import decay_ref as R
            sub = ch[:a.cpu_channels]
            R.emulator()        # built outside the timed window
            t0 = time.perf_counter()
            _, _, cst, cslots = R.emulate(S, sp["mass"], pT, phi, y, sub)
            ct = time.perf_counter() - t0
            _, cterms = work(sub, cst)
            out.update(cpu_channels=len(sub), cpu_threads=int(os.environ["OMP_NUM_THREADS"]), cpu_slots=cslots,
                       cpu_ms=round(ct * 1e3, 3), cpu_node_evals_per_s=cterms * points * 144 / ct)
        out["pi_plus_gain_at_lowest_pT"] = float(got[int(np.nonzero(mcids == 211)[0][0]), 0, 0, len(y) // 2] /
                                                 S[int(np.nonzero(mcids == 211)[0][0]), 0, 0, len(y) // 2])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
