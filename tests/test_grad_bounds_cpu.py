"""CPU side of the per-Gaussian gradient bound (tests/grad_bounds.py): everything the GPU test relies on is established
here against references only -- the oracle's gradients do not depend on the new exports, the float64 numpy chain and the
oracle agree within the bound, the pixel mask stays under its cap, K covers four times what the calibration builds
measure, and the bound is tight enough to notice the loss of any single Gaussian's gradient. The product's own math,
compiled for the host (tests/host_check), is then held to the same bound as the GPU will be."""
import numpy as np
import pytest

import grad_bounds as gb
from oracle import oracle as orc

CASES = list(gb.CASES)


@pytest.mark.parametrize("case", CASES)
def test_export_leaves_the_oracles_gradients_bit_identical(case):
    r = gb.reference(case)
    plain = r["R"].backward(r["gc"], r["gd"], r["ga"])
    assert set(plain) == set(r["G"])
    for k in plain:
        np.testing.assert_array_equal(plain[k], r["G"][k], err_msg=k)
    # the signed accumulators of the export are the sums the float32 outputs were rounded from
    np.testing.assert_array_equal(r["sums"][:, 0].astype(np.float32), r["G"]["means2D"][:, 0])
    np.testing.assert_array_equal(r["sums"][:, 1].astype(np.float32), r["G"]["means2D"][:, 1])
    # a magnitude sum is never below the magnitude of its signed sum: |sum u| coef <= coef sum |u|
    coef = r["R"].chain_state()[:, 12]
    assert np.all(np.abs(r["sums"][:, 7]) * coef <= r["unit"]["opacities"][:, 0] * (1 + 1e-12) + 1e-300)


def test_pixel_margins_agree_with_the_frame_margins():
    r = gb.reference("sh1_ragged")
    m = r["R"].pixel_margins()
    whole = r["R"].decision_margins()
    # the per-pixel margins are the frame's divided by max(1, magnitude of the exponent's terms): never larger
    assert m[..., 0].min() <= whole["alpha"] and m[..., 1].min() <= whole["T"]
    assert whole["power"] == (m[..., 2].min() if m[..., 2].min() < 1e-3 else 1e30)   # the frame form looks below 1e-3 only
    # masked pixels carry no upstream gradient, unmasked ones keep theirs
    mask = r["mask"]
    assert mask.any() and float(r["gc"][:, mask].abs().max()) == 0.0 and float(r["gd"][:, mask].abs().max()) == 0.0
    assert float(r["gc"][:, ~mask].abs().min()) > 0.0


@pytest.mark.parametrize("case", CASES)
def test_mask_share_is_below_the_cap(case):
    r = gb.reference(case)
    print(case, f"masked pixels: {r['share']:.4%}")
    assert r["share"] <= gb.MASK_CAP


@pytest.mark.parametrize("case", CASES)
def test_numpy_chain_agrees_with_the_oracle_within_the_bound(case):
    r = gb.reference(case)
    for k, ref in r["G"].items():
        e = gb.in_units(r["chain64"][k], ref, r["unit"][k])
        print(case, k, f"float64 chain vs oracle: {e.max():.3g} units at Gaussian {int(e.argmax())}, K = {gb.k_of(case, k):g}")
        assert e.max() <= gb.k_of(case, k), (k, int(e.argmax()))
        assert np.all(r["unit"][k] >= np.abs(r["chain64"][k]) * (1 - 1e-6)), k   # a unit is never below its value


@pytest.mark.parametrize("case", CASES)
def test_k_covers_four_times_the_calibration_builds(case):
    """K is chosen from references only: re-measure the float32-sum build, the exp-jitter build and the float64 chain."""
    got = gb.measure(case)
    assert set(got) == set(gb.K_TABLE[case])
    for k, (accf, jit, chain64) in got.items():
        tab = gb.K_TABLE[case][k]
        print(case, k, f"accf {accf:.3g} jit {jit:.3g} chain64 {chain64:.3g} units (table {tab[:3]}), K = {tab[3]:g}")
        assert 4.0 * max(accf, jit, chain64) <= tab[3], k
        assert tab[3] == gb.choose_k(max(tab[:3])), k      # the table's K follows from the table's own maxima


@pytest.mark.parametrize("case", CASES)
def test_a_lost_gaussian_violates_the_bound(case):
    seen, total = gb.detectable(case)
    print(case, f"{seen} of {total} Gaussians with a gradient would be noticed if it were zero ({seen / total:.2%})")
    assert total > 0 and seen >= 0.99 * total


@pytest.mark.parametrize("case", CASES)
def test_a_dropped_record_violates_the_bound(case):
    """The backward writes one gradient record per (Gaussian, 8x8 tile). By linearity, the oracle with the upstream gradients
    of one such tile zeroed is the result of an implementation that lost every record of that tile: the bound has to notice
    it for the Gaussians concerned. (Not for all of them by construction: a record whose whole contribution lies below
    K 2^-23 units of its Gaussian -- the rim of a large splat, alpha just above 1/255 on a few pixels -- is below the
    resolution any float32 comparison has. Nine in ten is asked for; the runs that chose the cases showed 92 .. 100 %.)"""
    r = gb.reference(case)
    N, H, W = r["R"].N, r["frame"]["H"], r["frame"]["W"]
    rng = np.random.default_rng(0)
    dropped = noticed = 0
    for _ in range(4):
        ty, tx = int(rng.integers(0, (H + 7) // 8)), int(rng.integers(0, (W + 7) // 8))
        ups = [None if t is None else t.clone() for t in (r["gc"], r["gd"], r["ga"])]
        for t in ups:
            if t is not None:
                t[:, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = 0
        G2 = r["R"].backward(*ups)
        changed, seen = np.zeros(N, bool), np.zeros(N, bool)
        for k, ref in r["G"].items():
            changed |= (G2[k].reshape(N, -1) != ref.reshape(N, -1)).any(axis=1)
            seen |= gb.in_units(G2[k], ref, r["unit"][k]) > gb.k_of(case, k)
        dropped += int(changed.sum())
        noticed += int((seen & changed).sum())
    print(case, f"{noticed} of {dropped} dropped records noticed")
    assert dropped > 0 and noticed >= 0.9 * dropped


def test_in_units_edge_cases():
    ref = np.array([[1.0, 0.0], [0.0, 0.0]])
    unit = np.array([[2.0, 0.0], [0.0, 0.0]])
    assert gb.in_units(ref, ref, unit).tolist() == [0.0, 0.0]
    e = gb.in_units(ref + np.array([[2.0 * gb.EPS, 0.0], [0.0, 1e-30]]), ref, unit)
    assert e[0] == pytest.approx(1.0) and np.isinf(e[1])     # anything where the unit is zero is out of bound


def test_record_counts_reach_every_summation_route():
    """The scenes named after the backward's summation routes have Gaussians on them (8x8-tile counts of the host
    emulation = gradient records per Gaussian): <= COOP = 32 records on both sides of the threshold, BWD_BIG = 2 048 on
    both sides, chunk counts that are not multiples of BWD_CHUNK = 1 024."""
    d = gb.record_counts("mixed_coop")[gb.has_gradient("mixed_coop")]      # of the Gaussians that receive a gradient
    assert {31, 32, 33} <= set(d.tolist())
    assert ((d > 32) & (d <= 2048)).any() and (d > 2048).any()
    d = gb.record_counts("screen_filling")
    assert (d > 2048).sum() >= 20 and ((d > 2048) & (d % 1024 != 0)).any()


@pytest.mark.parametrize("case", CASES)
def test_host_emulation_of_the_product_math_meets_the_bound(case):
    """The product's per-pixel and per-Gaussian math (raster_math.h compiled for the host: exp2 in the log2 domain, fused
    multiply-adds, the one-scalar recurrence, float32 sums) is held to the bound the GPU is held to."""
    import hostcheck
    r = gb.reference(case)
    g = r["g"]
    h = hostcheck.render(r["frame"], g["means3D"], g["scales"], g["rotations"], g["opacities"], g["colors_precomp"],
                         g["shs"], r["gc"], r["gd"], r["ga"], backward=True)
    np.testing.assert_array_equal(h["radii"], r["R"].radii)
    for k, ref in r["G"].items():
        e = gb.in_units(h["grads"][k], ref, r["unit"][k])
        print(case, k, f"host emulation vs oracle: {e.max():.3g} units at Gaussian {int(e.argmax())}, K = {gb.k_of(case, k):g}")
        assert e.max() <= gb.k_of(case, k), (k, int(e.argmax()), float(e.max()))
