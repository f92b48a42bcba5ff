"""Shared by tests/test_guided_cpu.py and tests/test_gpu_guided.py: the contaminated scene of the guided sampler's end-to-end test and its seeds."""
import numpy as np

# The 400-match, 65 %-outlier scene of the end-to-end test.  The quality is the inlier indicator plus N(0, USE_SIGMA), USE_SIGMA a quarter of the
# distance between the two classes.  The seeds are picked by the numpy twins alone, before anything runs on a GPU: among the generator seeds 61 .. 72 and
# the call seeds 1 .. 5, the first pair (in that order) for which the uniform sampler's 64 seven-point samples contain no all-inlier sample and the guided
# sampler's contain the most -- here all 64 -- because one all-inlier sample of the noise-sensitive seven-point solver is often not enough for a pose
# (tests/test_guided_cpu.py keeps the check that the issue asks for: none against at least five).
USE_N, USE_SHARE, USE_GEN_SEED, USE_CALL_SEED, USE_N_HYP, USE_GROWTH, USE_SIGMA = 400, 0.65, 61, 1, 64, 64, 0.25


def contaminated(n, share, gen_seed):
    """the recipe of tools/config4_ransac.py (tests/test_gpu_adaptive.py::_contaminated): 0.5 px noise, `share` of the matches displaced by U(20, 80) px
    in views 2 and 3.  -> scene (n, 6), CalM (9, 3), inlier (n,) bool"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, int(share * n), replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    inlier = np.ones(n, dtype=bool)
    inlier[bad] = False
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM), inlier


def use_case():
    """scene, CalM, inlier flags and the quality of the end-to-end test: the inlier indicator plus Gaussian noise"""
    scene, calm, inlier = contaminated(USE_N, USE_SHARE, USE_GEN_SEED)
    quality = inlier.astype(np.float64) + np.random.default_rng(USE_GEN_SEED + 200).normal(0.0, USE_SIGMA, USE_N)
    return scene, calm, inlier, quality


def eight():
    """the eight scenes of tests/test_gpu_adaptive.py::_eight: noise-free 200 | 400 with 20, 35, 50, 65 % outliers | 200 random matches | 5 matches | a
    fountain triplet with more than 300 matches; a CalM each.  -> (list of (n, 6) arrays, (8, 9, 3) CalMs)"""
    import os
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, 200, noise=0.0, seed=31)
    items = [(np.ascontiguousarray(C[0]), np.ascontiguousarray(CalM))]
    items += [contaminated(400, share, 41 + k)[:2] for k, share in enumerate((0.20, 0.35, 0.50, 0.65))]
    items.append((np.ascontiguousarray(np.random.default_rng(5).uniform(0, 1000, (200, 6))), items[0][1]))
    items.append((contaminated(400, 0.25, 51)[0][:5].copy(), items[0][1]))
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epfl_all.npz"))
    off, K, trip = d["fountain_offsets"], d["fountain_K"], d["fountain_triplets"]
    t = int(np.nonzero(np.diff(off) > 300)[0][0])
    items.append((np.ascontiguousarray(d["fountain_corresp"][off[t]:off[t + 1]]), np.concatenate([K[v - 1] for v in trip[t][:3]], axis=0)))
    return [a for a, _ in items], np.stack([c for _, c in items])
