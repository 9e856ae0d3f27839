"""Wavefront balance of the F_TS k_spectra workgroups: mean / max wavefront cost per composition of
64-task blocks (one wavefront each; task = class + nclass q) into workgroups, on a cell sample of BASELINE config 2
(SMASH as integrand classes, Grad, 48 pT x 32 phi x 21 y).  CPU only: the per-lane kinds come from the host build of
the device math (tests/native/cf_emulator.cpp), the per-wavefront votes are taken as sep_setup takes them.
usage: python tools/wg_census.py [cells] [--pT i,j,...]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import emu_spectra, emulator  # noqa: E402
from is3d2_amd import make_spec, synth  # noqa: E402

# VALU instructions of one wavefront on one cell: the lane setup, then the phi loop of a
# Boltzmann-tail / near-tail / normal wavefront; a wavefront whose lanes all skip the cell branches past both (an
# estimate, 7.3 does not list it)
SETUP, TAIL, NEAR, NORMAL, SKIP = 53, 174, 263, 356, 6


def block_costs(spec, surf):
    """[pT][cell][block] cost of each 64-task wavefront of the Grad F_TS launch; returns (cost, nclass, ntask)."""
    n = len(surf["tau"])
    npT, ns, nq = len(spec["pT"]), len(spec["species"]["mass"]), len(spec["y"])
    buf = np.zeros(npT * n * ns * nq, dtype=np.int8)
    emulator().emu_set_census_lanes(buf.ctypes.data_as(C.c_void_p))
    try:
        emu_spectra(spec, surf, variant=3)
    finally:
        emulator().emu_set_census_lanes(None)
    buf = buf.reshape(npT, n, ns, nq)
    key = list(zip(spec["species"]["mass"], spec["species"]["sign"], spec["species"]["baryon"]))
    rep, seen = [], set()
    for i, k in enumerate(key):
        if k not in seen:
            seen.add(k)
            rep.append(i)
    nc = len(rep)
    ntask = nc * nq
    nblk = -(-ntask // 64)
    cat = np.transpose(buf[:, :, rep, :], (0, 1, 3, 2)).reshape(npT, n, ntask)      # task = class + nclass q
    cat = np.concatenate([cat, np.zeros((npT, n, nblk * 64 - ntask), np.int8)], axis=2).reshape(npT, n, nblk, 64)
    # lane codes (cf_emulator.cpp): 0 no lane / dead cell, 1 skipped, 2 tail, 3 normal, 4 near-tail; the device votes
    # per wavefront: tail if every live lane is, else near if every live lane is near or tail, else the normal fours
    cell_live = (cat > 0).any(axis=(2, 3))[:, :, None]
    has_t, has_f, has_n = (cat == 2).any(axis=3), (cat == 3).any(axis=3), (cat == 4).any(axis=3)
    loop = np.where(has_f, NORMAL, np.where(has_n, NEAR, TAIL))
    cost = np.where(has_t | has_f | has_n, SETUP + loop, SKIP) * cell_live
    return cost.astype(np.int64), nc, ntask


def rows_of(blocks, npart, ntask):
    """distinct q rows (task // npart) the tasks of these blocks touch"""
    rows = set()
    for b in blocks:
        t0, t1 = 64 * int(b), min(ntask, 64 * int(b) + 64) - 1
        if t1 >= t0:
            rows.update(range(t0 // npart, t1 // npart + 1))
    return rows


def balance(cost, m, W, tile=12):
    """mean / max wavefront cost over the workgroups of map m, the waves meeting at every tile of `tile` cells: the
    sum of the per-(workgroup, tile) means over the sum of the maxima.  cost: [cell][block]."""
    n, nblk = cost.shape
    pad = -n % tile
    c = np.concatenate([cost, np.zeros((pad, nblk), cost.dtype)]) if pad else cost
    t = c.reshape(-1, tile, nblk).sum(axis=1)[:, np.asarray(m)].reshape(-1, nblk // W, W)      # [tile][wg][wave]
    return float(t.mean(axis=2).sum() / max(1, t.max(axis=2).sum()))


def sorted_map(total, window=None):
    """blocks ordered by falling cost inside windows of `window` consecutive blocks (None: the whole pT)"""
    nblk = len(total)
    window = window or nblk
    m = []
    for b0 in range(0, nblk, window):
        ids = np.arange(b0, min(nblk, b0 + window))
        m.extend(ids[np.argsort(-total[ids], kind="stable")])
    return np.asarray(m)


def capped_map(total, W, npart, ntask, cap):
    """... inside the longest runs of whole workgroups whose tasks stay within `cap` q rows: the composition the
    rejected device planner wrote (every workgroup within the rows its LDS tables hold)"""
    nblk = len(total)
    m, b0 = [], 0
    while b0 < nblk:
        b1 = min(nblk, b0 + W)
        while b1 + W <= nblk and len(rows_of(range(b0, b1 + W), npart, ntask)) <= cap:
            b1 += W
        ids = np.arange(b0, b1)
        # a run of one workgroup is the consecutive workgroup: nothing to regroup
        m.extend(ids[np.argsort(-total[ids], kind="stable")] if b1 - b0 > W else ids)
        b0 = b1
    return np.asarray(m)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("cells", nargs="?", type=int, default=240)
    ap.add_argument("--pT", default="", help="comma-separated pT indices (default: all 48)")
    a = ap.parse_args()
    n = a.cells
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=1, dimension=3, pT="pT48", phi="phi32", y="y21")
    if a.pT:
        sel = [int(x) for x in a.pT.split(",")]
        spec["pT"], spec["pT_w"] = spec["pT"][sel].copy(), spec["pT_w"][sel].copy()
    s = synth.as_read(synth.surface(n, seed=7, dimension=3, full3d=True))
    cost, nc, ntask = block_costs(spec, s)
    npT, _, nblk = cost.shape
    print("%d cells, %d classes, %d tasks, %d blocks per pT" % (n, nc, ntask, nblk))
    print("mean VALU per cell of the first six blocks: " + " ".join("%.0f" % v for v in cost.mean(axis=(0, 1))[:6]))
    for W in (4, 6, 8):
        nb = -(-ntask // (64 * W)) * W
        c = np.concatenate([cost, np.zeros((npT, cost.shape[1], nb - nblk), cost.dtype)], axis=2) if nb > nblk else cost
        rmin = min(-(-ntask // nc), (64 * W - 1) // nc + 2)      # rows W consecutive blocks can touch
        rows = {"consecutive": (lambda t: np.arange(nb)), "cost-sorted per pT": (lambda t: sorted_map(t)),
                "cost-sorted, windows of 12": (lambda t: sorted_map(t, 12))}
        for cap in range(rmin, rmin + 3):
            rows["cost-sorted within %d q rows" % cap] = (lambda t, cap=cap: capped_map(t, W, nc, ntask, cap))
        print("%d-wave workgroups:" % W)
        for name, f in rows.items():
            num = np.zeros(2)
            mr, worst = 0, 1.0
            maps = [f(c[i].sum(axis=0)) for i in range(npT)]
            if name != "consecutive" and all(np.array_equal(m, np.arange(nb)) for m in maps):
                continue      # a row cap that admits no run longer than one workgroup: the consecutive composition
            for i, m in enumerate(maps):
                assert np.array_equal(np.sort(m), np.arange(nb))
                b = np.array([balance(c[i], m, W), balance(c[i], m, W, tile=c.shape[1])])
                worst = min(worst, b[0])
                num += b * c[i].sum()
                mr = max(mr, max(len(rows_of(m[g:g + W], nc, ntask)) for g in range(0, nb, W)))
            num /= max(float(c.sum()), 1.0)
            print("  %-30s mean/max per 12-cell tile %.3f (worst pT %.3f), over the sample %.3f, max q rows %d"
                  % (name, num[0], worst, num[1], mr))


if __name__ == "__main__":
    main()
