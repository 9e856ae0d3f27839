#!/usr/bin/env python3
"""Record what a checkout WITHOUT four-body channels computes for tests/decay4_ref.parent_cases(), into
tests/golden/decay4_parent_<name>.npz: the Monte Carlo channel table, the plan statistics, the feed-down of a small
grid and the decayed list of a short primary list, all from that checkout's own CPU emulators
(tests/native/decay_emulator.cpp, decay_list_emulator.cpp over its headers).  tests/test_decay4_cpu.py compares the
three-slot call of this tree against them byte for byte.

    python tools/record_decay_parent.py <checkout of the commit before is3d_set_decays4> [out_dir]
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main(checkout, out_dir):
    sys.path[:0] = [os.path.join(checkout, "tests"), checkout]
    import decay_list_ref as L        # the checkout's: they build the emulators from the checkout's headers
    import decay_ref as R
    assert os.path.realpath(R.ROOT) == os.path.realpath(checkout)
    spec = importlib.util.spec_from_file_location("decay4_ref", os.path.join(ROOT, "tests", "decay4_ref.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    for name, (mass, ch, S, pT, phi, y, prim, offsets, seed) in D.parent_cases().items():
        fd, ab, st, slots = R.emulate(S, mass, pT, phi, y, ch)
        out, off, origins, lst, pst = L.emulate(mass, ch, prim, offsets, seed)
        kept, level = L.mc_channels(mass, ch)
        ints = np.array([[c["parent"], c["nbody"]] + c["d"] for c in kept], dtype=np.int32).reshape(-1, 5)
        dbls = np.array([[c["cum"], c["M"]] + c["m"] + c["k"] for c in kept], dtype=np.float64).reshape(-1, 8)
        keys = [k for k in sorted(st) if k != "ms_total"]
        np.savez_compressed(os.path.join(out_dir, "decay4_parent_%s.npz" % name), feeddown=fd, sum_abs=ab, slots=slots,
                            plan_stats=np.array([float(st[k]) for k in keys]), plan_stat_keys=np.array(keys),
                            list=out.view(np.uint8), offsets=off, origins=origins,
                            list_stats=np.array([lst[k] for k in L.STAT_KEYS], dtype=np.int64),
                            chan_ints=ints, chan_dbls=dbls, level=level)
        print(name, "kept", st["kept"], "levels", st["levels"], "finals", len(out))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden"))
