#!/usr/bin/env python
"""Sample + decay in one device-resident pass (is3d_sample_decayed) against the two calls it replaces, on
one GPU, in one process and one build.

Shape: tools/decay_list_bench.py's defaults -- the SMASH decay table (tests/golden/decays_smash.npz, 444 chosen species),
a synthetic 2+1D surface of --cells cells (df_mode 2) and as many events as give about --primaries primaries (from a
two-event trial).  Two pairs, the legs of a pair alternating: `warmup` untimed rounds, then `repeats` timed ones.

  pair "list":    sample + decay_sampled(bin = 0)                       against  sample_decayed(list = 1, bin = 0)
  pair "binned":  sample_binned(keep_list = 1) + decay_sampled(bin = 1)  against  sample_decayed(list = 0, bin = 1)

The host clock is taken around the C calls alone (each ends synchronised; reading the list back through the getters is
outside the window on both sides).  Every repeat asserts that the two legs agree: the records, offsets and origins of
the list pair byte for byte, the histogram words of the binned pair.  One JSON line: per leg the median, range and every
repeat of the wall time, the device time of the decay stage (decay_list_stats ms_total) and the two transfer counters
("list_h2d_bytes", "list_d2h_bytes"; for the two-call legs the sum of both calls); the speed-up of each pair from the
medians; is3d_build_id().

    python tools/sample_decay_bench.py [--repeats 5] [--warmup 1] [--primaries 1000000] [--cells 1000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = dict(pT_min=0.0, pT_max=3.0, pT_bins=12, y_cut=2.0, y_bins=10, phip_bins=12, eta_cut=3.0, eta_bins=12,
            tau_min=0.0, tau_max=12.0, tau_bins=6, r_min=0.0, r_max=12.0, r_bins=6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--primaries", type=int, default=1_000_000)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    from is3d2_amd import _lib, build_engine, hrg, make_spec, surface_averages, synth
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "decays_smash.npz")))
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=2, dimension=2)
    ch = hrg.decay_channels(d, d, spec["species"]["mcid"])
    s = synth.as_read(synth.surface(a.cells, seed=a.seed))
    plasma = np.ascontiguousarray(surface_averages(s, 0), dtype=np.float64)
    e = build_engine(spec, s, T_avg=plasma[0])
    e.set_decays(ch)
    e.set_sample_bins(**BINS)
    trial, _, _ = e.sample(a.seed, 2, 0.5, 0, plasma)
    nev = max(1, int(round(a.primaries / max(len(trial) / 2.0, 1.0))))
    sp = _lib.SampleParams(a.seed, nev, 0, 0.5)
    pl = plasma.ctypes.data_as(C.POINTER(C.c_double))
    lib, h = e.lib, e._e
    e._list_events = nev

    def chk(rc):
        if rc:
            raise RuntimeError(lib.is3d_last_error(h).decode())

    def timed(*calls):
        """wall ms around the calls, and the transfer counters summed over them"""
        h2d = d2h = 0
        t0 = time.perf_counter()
        for f in calls:
            chk(f())
            h2d += lib.is3d_get_tuning(h, b"list_h2d_bytes")
            d2h += lib.is3d_get_tuning(h, b"list_d2h_bytes")
        return 1e3 * (time.perf_counter() - t0), h2d, d2h

    def held_list():
        parts, origins = e._decayed_list()
        off = np.zeros(nev + 1, dtype=np.int64)
        chk(lib.is3d_sample_offsets(h, off.ctypes.data_as(C.POINTER(C.c_long))))
        return parts.tobytes(), off.tobytes(), origins.tobytes()

    legs = {
        "list_two_calls": lambda: timed(lambda: lib.is3d_sample(h, C.byref(sp), pl), lambda: lib.is3d_decay_sampled(h, a.seed, 0)),
        "list_one_call": lambda: timed(lambda: lib.is3d_sample_decayed(h, C.byref(sp), pl, a.seed, 1, 0)),
        "binned_two_calls": lambda: timed(lambda: lib.is3d_sample_binned(h, C.byref(sp), pl, 1), lambda: lib.is3d_decay_sampled(h, a.seed, 1)),
        "binned_one_call": lambda: timed(lambda: lib.is3d_sample_decayed(h, C.byref(sp), pl, a.seed, 0, 1)),
    }
    rec = {k: dict(wall=[], device=[], h2d=0, d2h=0) for k in legs}
    for r in range(a.warmup + a.repeats):
        got = {}
        for name, leg in legs.items():
            w, h2d, d2h = leg()
            st = e.decay_list_stats()
            got[name] = held_list() if name.startswith("list") else {k: v.tobytes() for k, v in e.sample_hist().items()}
            if r >= a.warmup:
                rec[name]["wall"].append(w)
                rec[name]["device"].append(st["ms_total"])
                rec[name].update(h2d=h2d, d2h=d2h, decay_batches=st["batches"], sample_batches=e.sample_stats()["batches"])
        assert got["list_two_calls"] == got["list_one_call"], "the lists of repeat %d differ" % r
        assert got["binned_two_calls"] == got["binned_one_call"], "the histograms of repeat %d differ" % r
    st = e.decay_list_stats()
    out = dict(cells=a.cells, events=nev, primaries=st["primaries"], decays=st["decays"], final_particles=st["final_particles"],
               passes=st["passes"], repeats=a.repeats, equal=True, build_id=_lib.build_id())
    for name, v in rec.items():
        out[name] = dict(wall_ms=round(float(np.median(v["wall"])), 3), wall_range=[round(min(v["wall"]), 3), round(max(v["wall"]), 3)],
                         wall_all=[round(x, 3) for x in v["wall"]], decay_device_ms=round(float(np.median(v["device"])), 3),
                         list_h2d_bytes=v["h2d"], list_d2h_bytes=v["d2h"], sample_batches=v["sample_batches"],
                         decay_batches=v["decay_batches"])
    for pair in ("list", "binned"):
        out[pair + "_speedup"] = round(out[pair + "_two_calls"]["wall_ms"] / out[pair + "_one_call"]["wall_ms"], 3)
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
