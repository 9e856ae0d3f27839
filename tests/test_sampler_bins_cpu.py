"""CPU tier of the sampler's test_sampler = 1 binned distributions: is3d2_amd/csrc/sampler_bins.h built for the host
(tests/native/sampler_bins_emulator.cpp) against a numpy restatement of BinSampledParticle.cpp:9-133, the fixed-point
vn sums, the results/sampled writers of host_io.cpp against a Python formatting, and the serial sampler binned."""
import numpy as np
import pytest

from is3d2_amd import make_spec, synth
from oracle import oracle as O

import sampler_bins_ref as B

TWO_PI = B.TWO_PI


def below(x):
    return np.nextafter(x, -np.inf)


def above(x):
    return np.nextafter(x, np.inf)


INDEX_CASES = [
    # (lo, width, bins): pT with pT_min > 0, a rapidity window, an angle, one bin
    (0.3, (2.1 - 0.3) / 12.0, 12),
    (-0.4, 2.0 * 0.4 / 10.0, 10),
    (0.0, TWO_PI / 8.0, 8),
    (1.5, 4.0, 1),
]


@pytest.mark.parametrize("lo,width,n", INDEX_CASES)
def test_bin_index_equals_the_numpy_restatement(lo, width, n):
    edges = lo + width * np.arange(n + 1)
    hi = lo + width * n
    v = np.concatenate([edges, below(edges), above(edges), [lo - 1.0, lo - 1e-300, -1e300, hi, above(hi), below(hi), 1e300,
                                                             np.inf, -np.inf, np.nan],
                        np.random.default_rng(5).uniform(lo - width, hi + width, 2000)])
    got = B.c_index(v, lo, width, n)
    want = B.np_index(v, lo, width, n)
    np.testing.assert_array_equal(got, want)
    assert got[np.isclose(v, lo - 1.0)].max() == -1                      # below the minimum
    assert B.c_index([lo], lo, width, n)[0] == 0                         # exactly on the first edge
    # a value whose quotient is exactly n is dropped, one just inside the last bin is kept
    q = np.array([hi, below(hi)])
    f = np.floor((q - lo) / width)
    np.testing.assert_array_equal(B.c_index(q, lo, width, n), np.where(f < n, f, -1))
    assert (got >= -1).all() and (got < n).all()


def test_a_particle_lands_where_the_reference_puts_it():
    """Whole particles through bin_particle: negative angles are wrapped, an angle that wraps to exactly 2 pi is dropped
    (index phip_bins), pT_min > 0 drops soft particles, each histogram drops on its own."""
    bins = dict(pT_min=0.2, pT_max=1.7, pT_bins=12, y_cut=0.4, y_bins=10, phip_bins=8, eta_cut=1.4, eta_bins=14, tau_min=1.0,
                tau_max=4.0, tau_bins=6, r_min=0.5, r_max=5.5, r_bins=5)
    rng = np.random.default_rng(11)
    n = 4000
    px, py = rng.normal(0, 0.6, n), rng.normal(0, 0.6, n)
    x, y = rng.normal(0, 3.0, n), rng.normal(0, 3.0, n)
    rap, eta, tau = rng.uniform(-0.6, 0.6, n), rng.uniform(-2.0, 2.0, n), rng.uniform(0.5, 4.5, n)
    # hand-made: on the axes, and py = -tiny with px > 0: atan2 = -tiny, + 2 pi rounds to 2 pi -> dropped from phip
    px[:6] = [1.0, -1.0, 0.0, 0.1, 1.0, 0.3]; py[:6] = [0.0, 0.1, 1.0, -1.0, -1e-300, -0.3]
    x[:6] = [2.0, -2.0, 0.0, 0.0, 2.0, 1.0]; y[:6] = [0.0, -0.0, 2.0, -2.0, -1e-300, -1.0]
    tau[:4] = [1.0, 4.0, below(4.0), below(1.0)]
    rap[:4] = [-0.4, 0.4, below(0.4), below(-0.4)]
    eta[:2] = [-1.4, 1.4]
    idx, vn = B.c_land(bins, rap, eta, px, py, tau, x, y)
    p = dict(px=px, py=py, x=x, y=y, tau=tau, eta=eta)
    for part, (v, (lo, w)) in enumerate(zip(B.coordinates(p, rap), B.ranges(bins))):
        np.testing.assert_array_equal(idx[:, part], B.np_index(v, lo, w, int(bins[B.PARTS[part][1]])), err_msg=B.PARTS[part][0])
    assert np.arctan2(py[4], px[4]) < 0 and np.arctan2(py[4], px[4]) + TWO_PI == TWO_PI
    assert idx[4, 2] == -1 and idx[4, 6] == -1                 # wrapped to exactly 2 pi: dropped
    assert idx[3, 2] == 6 and idx[1, 2] == 3                   # -1.47 -> 4.81 (bin 6 of 8); 3.04 (bin 3)
    assert list(idx[:4, 4]) == [0, -1, 5, -1] and list(idx[:2, 0]) == [0, -1] and list(idx[:2, 1]) == [0, -1]
    assert (idx == -1).any(axis=0).all() and (idx >= 0).any(axis=0).all()    # every histogram drops some, keeps some
    # the harmonics are quantised for every particle, whether its pT is in range or not
    h = B.c_harmonics(px, py)
    np.testing.assert_array_equal(vn, np.rint(h * 2.0 ** 32).astype(np.int64))


def test_harmonics_against_cos_and_sin_of_k_phi():
    """|delta| <= 1e-13: the recurrence accumulates a few ulp per step over seven steps and the argument error of
    2 pi 2^-53 is multiplied by k <= 7."""
    rng = np.random.default_rng(3)
    n = 10000
    pT = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), n))
    phi = rng.uniform(-np.pi, np.pi, n)
    px, py = pT * np.cos(phi), pT * np.sin(phi)
    got = B.c_harmonics(px, py)
    a = np.arctan2(py, px)
    k = np.arange(1, 8)[None, :]
    want = np.concatenate([np.cos(k * a[:, None]), np.sin(k * a[:, None])], axis=1)
    err = float(np.max(np.abs(got - want)))
    print("harmonics: max |delta| = %.3e over %d directions" % (err, n))
    assert err <= 1e-13
    np.testing.assert_array_equal(B.c_harmonics([0.0], [0.0])[0], [1.0] * 7 + [0.0] * 7)   # atan2(0, 0) = 0


def test_fixed_point_sums_are_order_free_and_within_half_a_quantum_per_term():
    rng = np.random.default_rng(9)
    n = 200000
    v = np.cos(rng.uniform(0, TWO_PI, n))
    s = B.c_fixed_sum(v)
    exact = float(np.sum(v.astype(np.longdouble)))
    print("fixed-point sum of %d terms: %.17g, double sum %.17g, bound %.3e" % (n, s, exact, n * B.Q / 2))
    assert abs(s - exact) <= n * B.Q / 2
    for seed in (1, 2, 3):
        assert B.c_fixed_sum(rng.permutation(v)) == s
    assert B.c_fixed_sum(v[::-1].copy()) == s
    assert B.c_fixed_sum([1.0, -1.0, 0.5, 2.0 ** -33, 3 * 2.0 ** -33]) == 0.5 + 2 * B.Q      # ties to even: 0 and 2 q


def test_writers_match_the_reference_streams_byte_for_byte(tmp_path):
    """3 species, small bins, one empty pT bin (vn: 0 / 0 -> 0), Nevents = 3."""
    bins = dict(pT_min=0.1, pT_max=1.3, pT_bins=4, y_cut=0.75, y_bins=3, phip_bins=5, eta_cut=2.0, eta_bins=4, tau_min=0.5,
                tau_max=9.5, tau_bins=3, r_min=0.0, r_max=7.0, r_bins=2)
    rng = np.random.default_rng(21)
    npart, mcids = 3, [211, -321, 2212]
    hist = {name: rng.integers(0, 5000, (npart, int(bins[key]))) for name, key in B.PARTS}
    hist["pT_count"][1, 2] = 0
    hist["dN_dy"][2, :] = 0
    hist["dN_deta"][0, 1] = 123456789
    n = hist["pT_count"][None, :, :].astype(np.float64)
    hist["vn_real"] = rng.uniform(-0.3, 0.3, (7, npart, 4)) * n
    hist["vn_imag"] = rng.uniform(-0.3, 0.3, (7, npart, 4)) * n
    hist["vn_real"][:, 1, 2] = 0.0
    hist["vn_imag"][:, 1, 2] = 0.0
    hist["vn_real"][3, 0, 0] = 1e-9 * n[0, 0, 0]          # a small exponent in %.6e
    B.write_files(str(tmp_path), hist, bins, 3, mcids)
    got = B.read_tree(str(tmp_path / "results" / "sampled"))
    want = B.expected_files(hist, bins, 3, mcids)
    assert sorted(got) == sorted(want) and len(want) == 9 * npart
    for name in sorted(want):
        assert got[name] == want[name], name
    assert got["vn/vn_-321_test.dat"].splitlines()[2] == "8.500000e-01" + "\t0.000000e+00" * 7
    assert got["dN_dy/dN_dy_2212_average_test.dat"] == "0\n"
    # a second call overwrites (ios_base::out), it does not append
    B.write_files(str(tmp_path), hist, bins, 3, mcids)
    assert B.read_tree(str(tmp_path / "results" / "sampled")) == got


BINS_2D = B.TEST_BINS


@pytest.mark.parametrize("dimension,mode,fast", [(2, 1, 0), (3, 4, 1)])
def test_the_binned_emulator_equals_the_numpy_binning_of_its_own_list(dimension, mode, fast):
    nev, n, y_cut = 6, 200, 0.5
    spec = make_spec(chosen="pikp", df_mode=mode, dimension=dimension)
    s = synth.as_read(synth.surface(n, seed=23, dimension=dimension, full3d=(dimension == 3)))
    plasma = O.averages(s, 0)
    hist, st, p, drawn = B.sample_binned(spec, s, plasma, 11, nev, BINS_2D, y_cut=y_cut, fast=fast)
    npart = len(spec["species"]["mass"])
    assert st["kept"] == len(p) > 500
    rap = B.list_rapidity(p, dimension, drawn)
    assert B.ambiguous(p, rap, BINS_2D) == 0
    want = B.np_hist(p, rap, BINS_2D, npart)
    for name, _ in B.PARTS:
        np.testing.assert_array_equal(hist[name], want[name], err_msg=name)
        if "dphi" in name:
            assert hist[name].sum() == len(p), name             # the full circle
        else:
            assert 0 < hist[name].sum() < len(p), name          # the ranges cut into the populated region
    nbin = hist["pT_count"][None, :, :]
    for name in ("vn_real", "vn_imag"):
        assert (np.abs(hist[name] - want[name]) <= nbin * (B.Q / 2 + 1e-13)).all(), name
    if dimension == 2:      # the drawn rapidity is the one of (E, pz) to rounding
        assert np.max(np.abs(B.rapidity_from_momentum(p) - drawn)) < 1e-14
        np.testing.assert_array_equal(B.np_hist(p, B.rapidity_from_momentum(p), BINS_2D, npart)["dN_dy"], hist["dN_dy"])
