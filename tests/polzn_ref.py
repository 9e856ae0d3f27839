"""numpy restatement of the reference's spin-polarization loop (Polarization.cpp:98-255).

Every term is evaluated in float64 in the reference's expression order; the sum over cells (and, in 2+1D, over
the eta table) is accumulated in np.longdouble.  Returns the sums S[5] = (S_t, S_x, S_y, S_n, Snorm) and the
absolute sums A[5] = sum |term|, each [species][pT][phi][y] (y: one slot, y = 0, in 2+1D).

The spin components cancel (the vorticity's sign is random: |sum| / sum |term| down to ~1e-6), so parity is
measured as |got - ref| / sum |term|, never relative to the sum itself.

The vorticity of cell c is w[:, c] (the reference uses the index inside its 10 000-cell chunk,
Polarization.cpp:131-136: identical for the <= 10 000 cells used here).
"""
import numpy as np


def polarization(spec, surf, w, T_avg, lo=0, hi=None):
    """spec: make_spec dict; surf: surface dict; w: (6, n) wtx wty wtn wxy wxn wyn; cells [lo, hi)."""
    p = spec["params"]
    dim = p["dimension"]
    mass = np.asarray(spec["species"]["mass"], dtype=np.float64)
    sign = np.asarray(spec["species"]["sign"], dtype=np.float64)
    pT = np.asarray(spec["pT"], dtype=np.float64)
    phi = np.asarray(spec["phi"], dtype=np.float64)
    n = len(surf["tau"])
    hi = n if hi is None else hi
    T = np.float64(T_avg)
    if dim == 3:
        yv = np.asarray(spec["y"], dtype=np.float64)
        eta_w = np.ones(1)
    else:
        yv = np.zeros(1)
        eta = np.asarray(spec["eta"], dtype=np.float64)
        delta_eta = eta[1] - eta[0]                                   # :58
        eta_w = np.asarray(spec["eta_w"], dtype=np.float64) * delta_eta    # :68
    npart, npT, nphi, ny = len(mass), len(pT), len(phi), len(yv)
    cosphi, sinphi = np.cos(phi), np.sin(phi)
    shape = (npart, npT, nphi, ny)
    S = np.zeros((5,) + shape, dtype=np.longdouble)
    A = np.zeros((5,) + shape, dtype=np.longdouble)
    m_ = mass[:, None, None, None]
    s_ = sign[:, None, None, None]
    mT = np.sqrt(m_ * m_ + (pT * pT)[None, :, None, None])          # :151
    px = (pT[:, None] * cosphi[None, :])[None, :, :, None]             # :157
    py = (pT[:, None] * sinphi[None, :])[None, :, :, None]
    with np.errstate(over="ignore"):
        for c in range(lo, hi):
            tau = surf["tau"][c]
            tau2 = tau * tau
            dat, dax, day, dan = surf["dat"][c], surf["dax"][c], surf["day"][c], surf["dan"][c]
            ux, uy, un = surf["ux"][c], surf["uy"][c], surf["un"][c]
            ut = np.sqrt(np.abs(1.0 + ux * ux + uy * uy + tau2 * un * un))   # :126
            wtx, wty, wtn, wxy, wxn, wyn = (w[k][c] for k in range(6))
            mT_over_tau = mT / tau
            etas = [surf["eta"][c]] if dim == 3 else eta
            for ieta, e in enumerate(etas):
                dw = eta_w[ieta]
                d = (yv - e)[None, None, None, :]
                pt = mT * np.cosh(d)
                pn = mT_over_tau * np.sinh(d)
                tau2_pn = tau2 * pn
                pds = pt * dat + px * dax + py * day + pn * dan
                pdotu = pt * ut - px * ux - py * uy - tau2_pn * un
                f0 = 1.0 / (np.exp(pdotu / T) + s_)
                pref = -(1.0 / 8.0 / m_) * (1.0 - s_ * f0)
                spin = (pref * 2.0 * (wxy * pn - wxn * py + wyn * px),
                        pref * 2.0 * (wyn * pt - wtn * py + wty * pn),
                        pref * 2.0 * (-wxn * pt + wtn * px - wtx * pn),
                        pref * 2.0 * (wtx * py + wxy * pt - wty * px))
                for k in range(4):
                    term = dw * pds * f0 * spin[k]
                    S[k] += term
                    A[k] += np.abs(term)
                term = dw * pds * f0
                S[4] += term
                A[4] += np.abs(term)
    return S, A


def check_left_out(got, S, A, floor=1e-290):
    """What parity() leaves out is still checked: where every term of every cell overflowed in the reference
    (Snorm's sum |term| is 0: f0 = 1 / (inf + s) = 0 in each) all five outputs are exactly 0, and an output whose
    sum |term| is below the floor is itself no larger than the floor.  Returns the number of outputs left out."""
    got = np.asarray(got, dtype=np.float64).reshape(S.shape)
    gone = np.asarray(A[4] == 0)
    np.testing.assert_array_equal(got[:, gone], 0.0)
    low = np.asarray(A <= floor)
    assert np.all(np.abs(got[low]) <= floor * (1.0 + 1e-6))     # |got| <= (1 + parity bar) sum |term|
    return int(low.sum())


def parity(got, S, A, floor=1e-290):
    """(max |got - S| / A over A > floor, number of outputs left out)."""
    got = np.asarray(got, dtype=np.float64).reshape(S.shape)
    m = A > floor
    err = np.abs(got.astype(np.longdouble)[m] - S[m]) / A[m]
    return float(err.max()) if m.any() else 0.0, int((~m).sum())
