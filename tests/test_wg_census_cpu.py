"""CPU tier: tools/wg_census.py, the record behind DESIGN.md 3.22 (wavefront balance of the F_TS workgroups).  On a
small census of the config-2 grids (the emulator's lane kinds, four pT values, 36 cells) every composition the tool
prints is a permutation of the blocks, the row-capped ones keep each workgroup within the cap, and -- compared over
the whole sample, where consecutive W-tuples of a cost-sorted run minimise the sum of the workgroups' maxima over
every partition of that run -- none balances the wavefronts worse than the consecutive composition, at any pT."""
import importlib.util
import os

import numpy as np
import pytest

from is3d2_amd import make_spec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wg_census", os.path.join(ROOT, "tools", "wg_census.py"))
wg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wg)


@pytest.fixture(scope="module")
def census():
    spec = make_spec(hrg_eos=2, chosen="smash", df_mode=1, dimension=3, pT="pT48", phi="phi32", y="y21")
    sel = [0, 16, 32, 47]
    spec["pT"], spec["pT_w"] = spec["pT"][sel].copy(), spec["pT_w"][sel].copy()
    s = synth.as_read(synth.surface(36, seed=7, dimension=3, full3d=True))
    return wg.block_costs(spec, s)


def test_census_shape_and_costs(census):
    cost, nc, ntask = census
    assert nc == 193 and ntask == 4053 and cost.shape == (4, 36, 64)
    live = cost[cost > 0]
    assert set(np.unique(live)) <= {wg.SKIP, wg.SETUP + wg.TAIL, wg.SETUP + wg.NEAR, wg.SETUP + wg.NORMAL}
    # the light third of a q row costs more than the middle and heavy thirds (blocks 0, 1, 2 are row 0)
    m = cost.mean(axis=(0, 1))
    assert m[0] > m[1] and m[0] > m[2]


@pytest.mark.parametrize("W", [4, 6])
def test_compositions(census, W):
    cost, nc, ntask = census
    nb = -(-ntask // (64 * W)) * W
    c = np.concatenate([cost, np.zeros(cost.shape[:2] + (nb - cost.shape[2],), cost.dtype)], axis=2)
    rmin = min(-(-ntask // nc), (64 * W - 1) // nc + 2)
    ident = np.arange(nb)
    n = c.shape[1]
    for i in range(c.shape[0]):
        tot = c[i].sum(axis=0)
        b0 = wg.balance(c[i], ident, W, tile=n)
        maps = {"sorted": wg.sorted_map(tot), "w12": wg.sorted_map(tot, 12)}
        for cap in (rmin, rmin + 1, rmin + 2):
            maps[cap] = wg.capped_map(tot, W, nc, ntask, cap)
        for name, m in maps.items():
            assert np.array_equal(np.sort(m), ident), name
            if isinstance(name, int):
                assert max(len(wg.rows_of(m[g:g + W], nc, ntask)) for g in range(0, nb, W)) <= name
            if name != "w12" or 12 % W == 0:      # windows of 12 hold whole workgroups only when W divides 12
                assert wg.balance(c[i], m, W, tile=n) >= b0 - 1e-12, (i, name)
    assert np.array_equal(wg.capped_map(np.full(nb, 7), W, nc, ntask, rmin + 2), ident)      # equal costs: identity
