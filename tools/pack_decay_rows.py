#!/usr/bin/env python3
"""Pack the decay rows of the reference's PDG tables (data, not code) into the test fixtures

  tests/golden/decays_smash.npz          every row of PDG/pdg_smash.dat (1- and 2-body)
  tests/golden/decays_urqmd_subset.npz   the rows of PDG/pdg-urqmd_v3.3+.dat whose parent is lighter than
                                         URQMD_MASS_CUT GeV (they include 3- and 4-body channels)
  tests/golden/decays_urqmd_fourbody.npz every 4-body row of PDG/pdg-urqmd_v3.3+.dat with the particle records of
                                         their parents and daughters only

Format of a conventional PDG file (readindata.cpp:973-1007): per particle
  mcid name mass width gspin baryon strange charm bottom gisospin charge decays
followed by `decays` rows  mcid n_body branching d1 d2 d3 d4 d5.

Arrays: row_mcid, row_n_body, row_branching, row_daughters[n][5] (the rows, file order) and the particle records the
antiparticle rule and the masses need: p_mcid, p_mass, p_width, p_baryon, p_strange, p_charge (file order, no
antibaryons: is3d2_amd.hrg.decay_channels generates those).
"""
import os
import sys

import numpy as np

URQMD_MASS_CUT = 1.45


def read(path, mass_cut=None):
    toks = open(path, encoding="utf-8").read().split()
    parts, rows = [], []
    i = 0
    while i < len(toks):
        mcid, mass, width = int(toks[i]), float(toks[i + 2]), float(toks[i + 3])
        baryon, strange, charge, ndec = int(toks[i + 5]), int(toks[i + 6]), int(toks[i + 10]), int(toks[i + 11])
        parts.append((mcid, mass, width, baryon, strange, charge))
        i += 12
        for _ in range(ndec):
            if mass_cut is None or mass < mass_cut:
                rows.append((int(toks[i]), int(toks[i + 1]), float(toks[i + 2])) + tuple(int(v) for v in toks[i + 3:i + 8]))
            i += 8
    p = np.array(parts, dtype=object)
    r = np.array(rows, dtype=object)
    return dict(row_mcid=r[:, 0].astype(np.int64), row_n_body=r[:, 1].astype(np.int64),
                row_branching=r[:, 2].astype(np.float64), row_daughters=r[:, 3:8].astype(np.int64),
                p_mcid=p[:, 0].astype(np.int64), p_mass=p[:, 1].astype(np.float64), p_width=p[:, 2].astype(np.float64),
                p_baryon=p[:, 3].astype(np.int64), p_strange=p[:, 4].astype(np.int64), p_charge=p[:, 5].astype(np.int64))


def main(ref, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    d = read(os.path.join(ref, "PDG", "pdg_smash.dat"))
    np.savez_compressed(os.path.join(out_dir, "decays_smash.npz"), **d)
    print("smash: %d rows, bodies %s" % (len(d["row_mcid"]), sorted(set(d["row_n_body"].tolist()))))
    d = read(os.path.join(ref, "PDG", "pdg-urqmd_v3.3+.dat"), URQMD_MASS_CUT)
    np.savez_compressed(os.path.join(out_dir, "decays_urqmd_subset.npz"), **d)
    print("urqmd subset: %d rows, bodies %s" % (len(d["row_mcid"]), sorted(set(d["row_n_body"].tolist()))))
    d = read(os.path.join(ref, "PDG", "pdg-urqmd_v3.3+.dat"))
    rows = np.abs(d["row_n_body"]) == 4
    used = set(d["row_mcid"][rows].tolist()) | set(d["row_daughters"][rows][:, :4].ravel().tolist())
    parts = np.array([int(m) in used for m in d["p_mcid"]])
    d = {k: v[rows] if k.startswith("row_") else v[parts] for k, v in d.items()}
    np.savez_compressed(os.path.join(out_dir, "decays_urqmd_fourbody.npz"), **d)
    print("urqmd four-body: %d rows, summed branching %.4g, %d particle records" %
          (len(d["row_mcid"]), d["row_branching"].sum(), len(d["p_mcid"])))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "tests/golden")
