"""Hadron-resonance-gas species lists.

Mirrors the reference's PDG readers so the species arrays fed to the engine are
the ones iS3D builds from the same files:

* conventional format (hrg_eos = 1 UrQMD, 2 SMASH): readindata.cpp:973-1095 --
  every baryon row is followed by its antibaryon (-mcid, -baryon), and the
  quantum-statistics sign is -1 for even baryon number, +1 otherwise;
* smash-box format (hrg_eos = 3): readindata.cpp:1098-1215 with the
  mcid-digit decoding of read_mcid (readindata.cpp:736-969);
* chosen particles: first PDG entry with a matching mcid
  (EmissionFunction.cpp:356-372).

The numeric content of the PDG files is packed in is3d2_amd/data/pdg.npz by
tools/pack_reference_data.py.
"""
import os

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
HRG_NAMES = {1: "urqmd", 2: "smash", 3: "box"}


def _load():
    return np.load(os.path.join(_DATA, "pdg.npz"))


def read_mcid(mcid):
    """Spin degeneracy, baryon number, statistics sign, has-antiparticle from a PDG code."""
    x = abs(int(mcid))
    d = [(x // 10 ** i) % 10 for i in range(10)]
    nJ, nq3, nq2, nq1 = d[0], d[1], d[2], d[3]
    n8 = d[7]
    nJ = (nJ + n8) & 0xF                    # 4-bit bitfield in the reference
    is_deuteron = (mcid == 1000010020)
    is_hadron = (not is_deuteron) and nq3 != 0 and nq2 != 0
    is_meson = is_hadron and nq1 == 0
    is_baryon = is_hadron and nq1 != 0
    if is_hadron:
        spin = 0 if nJ == 0 else nJ - 1
    elif is_deuteron:
        spin = 2
    else:
        spin = nq3
    if is_hadron and nJ > 0:
        gspin = nJ
    elif is_deuteron:
        gspin = 3
    else:
        gspin = spin + 1
    if is_deuteron:
        baryon = 2
    elif is_hadron:
        baryon = 0 if is_meson else (1 if is_baryon else 0)
    else:
        baryon = 0
    if is_deuteron:
        sign = -1
    elif is_hadron:
        sign = -1 if is_meson else 1
    else:
        sign = spin % 2
    if is_hadron:
        has_anti = (baryon != 0) or (nq2 != nq3)
    elif is_deuteron:
        has_anti = True
    else:
        has_anti = (nq3 == 1)
    return gspin, baryon, sign, has_anti


def _c_mod2(b):
    return int(np.fmod(b, 2))


def pdg_particles(hrg):
    """Full particle list in reference order: dict of mcid, mass, gspin, baryon, sign arrays."""
    name = HRG_NAMES.get(hrg, hrg)
    d = _load()
    rows = []
    if name in ("smash", "urqmd"):
        for mcid, mass, gs, b in zip(d[name + "_mcid"], d[name + "_mass"], d[name + "_gspin"], d[name + "_baryon"]):
            rows.append((int(mcid), float(mass), int(gs), int(b)))
            if b > 0:
                rows.append((-int(mcid), float(mass), int(gs), -int(b)))
        sign = [(-1 if _c_mod2(b) == 0 else 1) for (_, _, _, b) in rows]
    elif name == "box":
        sign = []
        for mass, mcids in zip(d["box_mass"], d["box_mcids"]):
            for m in mcids:
                if m == 0:
                    continue
                gs, b, sg, anti = read_mcid(int(m))
                rows.append((int(m), float(mass), gs, b)); sign.append(sg)
                if anti:
                    rows.append((-int(m), float(mass), gs, -b)); sign.append(sg)
    else:
        raise ValueError("hrg_eos must be 1, 2 or 3")
    a = np.array(rows, dtype=object)
    return dict(mcid=a[:, 0].astype(np.int64), mass=a[:, 1].astype(np.float64),
                gspin=a[:, 2].astype(np.float64), baryon=a[:, 3].astype(np.float64),
                sign=np.array(sign, dtype=np.float64))


def decay_rows_with_antibaryons(rows, particles):
    """The decay rows and particle records of a conventional PDG file with the antibaryon entries the reference's
    reader generates (readindata.cpp:1013-1060): every baryon (baryon > 0) is followed by its antiparticle, whose
    rows repeat the baryon's with every daughter negated -- except daughters that are neutral non-strange mesons
    (baryon = charge = strange = 0, :1055), which are their own antiparticles.

    rows: dict of row_mcid, row_n_body, row_branching, row_daughters[n][5]; particles: dict of p_mcid, p_mass,
    p_width, p_baryon, p_strange, p_charge (file order).  Returns (rows, particles) in the same form."""
    info = {int(m): (int(b), int(s), int(q)) for m, b, s, q in
            zip(particles["p_mcid"], particles["p_baryon"], particles["p_strange"], particles["p_charge"])}
    by_parent = {}
    for m, nb, br, ds in zip(rows["row_mcid"], rows["row_n_body"], rows["row_branching"], rows["row_daughters"]):
        by_parent.setdefault(int(m), []).append((int(nb), float(br), [int(d) for d in ds]))
    out_rows, out_parts = [], []
    for k, m in enumerate(int(v) for v in particles["p_mcid"]):
        rec = [particles[f][k] for f in ("p_mass", "p_width", "p_baryon", "p_strange", "p_charge")]
        out_parts.append([m] + rec)
        for nb, br, ds in by_parent.get(m, []):
            out_rows.append((m, nb, br, ds))
        if rec[2] > 0:
            out_parts.append([-m, rec[0], rec[1], -rec[2], -rec[3], -rec[4]])
            for nb, br, ds in by_parent.get(m, []):
                anti = []
                for d in ds:
                    if d == 0:
                        anti.append(0)
                        continue
                    if d not in info:
                        raise ValueError("can not find decay particle %d for the anti-baryon of %d" % (d, m))
                    b, s, q = info[d]
                    anti.append(d if (b == 0 and q == 0 and s == 0) else -d)
                out_rows.append((-m, nb, br, anti))
    p = np.array(out_parts, dtype=object)
    new_parts = dict(p_mcid=p[:, 0].astype(np.int64), p_mass=p[:, 1].astype(np.float64),
                     p_width=p[:, 2].astype(np.float64), p_baryon=p[:, 3].astype(np.int64),
                     p_strange=p[:, 4].astype(np.int64), p_charge=p[:, 5].astype(np.int64))
    new_rows = dict(row_mcid=np.array([r[0] for r in out_rows], dtype=np.int64),
                    row_n_body=np.array([r[1] for r in out_rows], dtype=np.int64),
                    row_branching=np.array([r[2] for r in out_rows], dtype=np.float64),
                    row_daughters=np.array([r[3] for r in out_rows], dtype=np.int64).reshape(-1, 5))
    return new_rows, new_parts


def decay_channels(rows, particles, mcids, antibaryons=True, four_body=False):
    """The engine's channel table (_lib.DECAY_DTYPE, Engine.set_decays) for the chosen list `mcids` from PDG decay
    rows (the form above; antibaryons = True generates the antibaryon channels first).  A row whose parent is not
    chosen is dropped; a daughter that is not chosen gets index -1 (its mass and width still enter the kinematics);
    rows with more than three bodies keep their first three daughters (the engine skips and counts them).
    four_body = True: the table in _lib.DECAY4_DTYPE with the fourth daughter filled (Engine.set_decays then keeps
    the open 4-body channels); rows with more than four bodies keep their first four."""
    from ._lib import DECAY4_DTYPE, DECAY_DTYPE
    if four_body:
        DECAY_DTYPE = DECAY4_DTYPE
    slots = 4 if four_body else 3
    if antibaryons:
        rows, particles = decay_rows_with_antibaryons(rows, particles)
    rec = {}
    for m, mass, width in zip(particles["p_mcid"], particles["p_mass"], particles["p_width"]):
        rec.setdefault(int(m), (float(mass), float(width)))
    index = {}
    for i, m in enumerate(int(v) for v in mcids):
        index.setdefault(m, i)
    out = []
    for m, nb, br, ds in zip(rows["row_mcid"], rows["row_n_body"], rows["row_branching"], rows["row_daughters"]):
        m, nb = int(m), abs(int(nb))     # the UrQMD table flags some rows with a negative body count
        if m not in index:
            continue
        c = np.zeros((), dtype=DECAY_DTYPE)
        c["parent"], c["n_body"], c["branching"] = index[m], nb, br
        c["mass_parent"], c["width_parent"] = rec[m]
        c["daughter"] = -1
        for k in range(min(nb, slots)):
            d = int(ds[k])
            if d not in rec:
                raise ValueError("decay row of %d: daughter %d is not in the particle list" % (m, d))
            c["daughter"][k] = index.get(d, -1)
            c["mass"][k], c["width"][k] = rec[d]
        out.append(c)
    return np.array(out, dtype=DECAY_DTYPE) if out else np.zeros(0, dtype=DECAY_DTYPE)


def chosen_mcids(name):
    return _load()["chosen_" + name].copy()


def chosen_species(particles, mcids):
    """Species arrays (mass, sign, degeneracy, baryon, mcid) for the chosen MCIDs."""
    idx = []
    for m in mcids:
        hit = np.nonzero(particles["mcid"] == m)[0]
        if len(hit) == 0:
            raise ValueError("chosen particle %d not in PDG list" % m)
        idx.append(hit[0])
    idx = np.array(idx)
    return dict(mass=particles["mass"][idx].copy(), sign=particles["sign"][idx].copy(),
                degen=particles["gspin"][idx].copy(), baryon=particles["baryon"][idx].copy(),
                mcid=particles["mcid"][idx].copy())


# the ten delta-f coefficient files of deltaf_coefficients/vh/<list>/ in table order, with the reference's label columns
DF_FILES = [("c0", "c0_T4 [fm^3/GeV^3 * GeV^4]"), ("c1", "c1_T3 [fm^3/GeV^2 * GeV^3]"), ("c2", "c2_T4 [fm^3/GeV^3 * GeV^4]"),
            ("c3", "c3_T4 [fm^3/GeV * GeV^4]"), ("c4", "c4_T5 [fm^3/GeV^2 * GeV^5]"), ("F", "F_over_T [fm^-1 / GeV]"),
            ("G", "G [1]"), ("betabulk", "betabulk_over_T4 [fm^-4 / GeV^4]"), ("betaV", "betaV_over_T3 [fm^-3 / GeV^3]"),
            ("betapi", "betapi_over_T4 [fm^-4 / GeV^4]")]


def write_df_tables(dir, T, muB, tab, digits=6):
    """Write tab[10][nmuB][nT] (Engine.generate_df_tables, data.df_tables) as the ten files c0.dat .. betapi.dat in
    `dir`, in the format of the reference's generator (deltaf_table.cpp:122-133, 240-244), which the reference itself
    and a run directory read: line 1 nT, line 2 nmuB, the label line, then rows "T  muB  value" with muB outer and T
    inner, fixed with `digits` decimals (the reference: 6; 17 keeps every bit of the grid and of values near 1)."""
    T, muB = np.asarray(T, dtype=np.float64), np.asarray(muB, dtype=np.float64)
    tab = np.asarray(tab, dtype=np.float64).reshape(10, len(muB), len(T))
    os.makedirs(dir, exist_ok=True)
    row = "%%8.%df\t\t%%.%df\t\t%%.%df\n" % (digits, digits, digits)
    for k, (name, label) in enumerate(DF_FILES):
        with open(os.path.join(dir, name + ".dat"), "w") as f:
            f.write("%d\n%d\nT [GeV]\t\tmuB [GeV]\t\t%s\n" % (len(T), len(muB), label))
            for iB in range(len(muB)):
                for iT in range(len(T)):
                    f.write(row % (T[iT], muB[iB], tab[k, iB, iT]))
