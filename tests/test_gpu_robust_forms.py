"""
The robust estimators' call layer (csrc/capi.hip: one ScenesCall, robust_dev / robust_host, reserve_robust), form by form.

(a) every refusal of every scene-list form, by return code and by the exact tff_last_error() text -- the texts are written out below as the library has
    always spelled them, not read back from it -- with the outputs keeping a canary;
(b) one context reused across forms of different sizes (fixed, guided + adaptive + MSAC, fixed again): both fixed results bit for bit equal, and each
    result that of a fresh context -- the workspaces are laid out once per call and reserved before its first launch;
(c) more candidates (C = S * n_cand = 640) than rows in a chunk: scene s still equals its own one-scene call bit for bit -- the retry list of the row
    kernels is sized for the candidates' re-draw before the call starts.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MASK64 = (1 << 64) - 1
E_INVALID = -10001

M_METHOD = "robust estimation: the method must be TFF_METHOD_LINEAR_TFT or TFF_METHOD_LINEAR_F"
M_NSAMPLE = "robust estimation: n_sample must be 0 or between the method's minimum (7 / 8) and 16"
M_NHYP = "robust estimation: n_hyp must be between 1 and 2^31 - 1"
M_NCAND = "robust estimation: n_cand must be between 1 and 64"
M_LO = "robust estimation: lo_rounds must be between 0 and 8"
M_THR = "robust estimation: the threshold must be a positive finite number"
M_NULL = "null pointer"
M_NULL_OFF = "null offsets"
M_S = "robust estimation: negative number of scenes"
M_NTOTAL = "robust estimation: n_total must be between 0 and 2^31 - 1"
M_NSMAX = "robust estimation: ns_max must be between 0 and 2^24"
M_STRIDE = "calm_stride must be 0 (shared CalM) or 27"
M_SHYP = "robust estimation: S * n_hyp above 2^31 - 1"
M_SCAND = "robust estimation: S * n_cand above the ragged call's 2^28 - 1 items"
M_ROWS = "ragged batches run on the row kernels: TFF_OPT_ROWS = 0 is not supported"
M_KERNEL = "ragged batches: TFF_OPT_KERNEL = 1 (fused single-wavefront kernels) is not supported"
M_CONF = "robust estimation: the confidence must lie strictly between 0 and 1"
M_FIRST = "robust estimation: first_round must be a multiple of 4 and at least 4"
M_ORDER = "guided sampling: null order"
M_GROWTH = "guided sampling: growth must be between 1 and 2^31 - 2^25"
M_NEG_OFF = "robust estimation: negative offset"
M_DECREASING = "robust estimation: decreasing offsets"
M_SCENE_BIG = "robust estimation: a scene of more than 2^24 correspondences"

OUTPUTS = ("Rt2", "Rt3", "T", "mask", "info", "status")
# the bad-argument list of tests/test_gpu_robust_scenes.py::test_refusals with the text each one is refused with
BAD = [(dict(method=1), M_METHOD), (dict(method=7), M_METHOD), (dict(method=-1), M_METHOD), (dict(n_sample=6), M_NSAMPLE),
       (dict(method=6, n_sample=7), M_NSAMPLE), (dict(n_sample=17), M_NSAMPLE), (dict(n_hyp=0), M_NHYP), (dict(n_hyp=-5), M_NHYP),
       (dict(n_cand=0), M_NCAND), (dict(n_cand=65), M_NCAND), (dict(lo_rounds=-1), M_LO), (dict(lo_rounds=9), M_LO), (dict(threshold=0.0), M_THR),
       (dict(threshold=float("nan")), M_THR), (dict(threshold=float("inf")), M_THR), (dict(scenes=None), M_NULL), (dict(calm=None), M_NULL),
       (dict(offsets=None), M_NULL_OFF), (dict(S=-1), M_S), (dict(S=3, n_hyp=(1 << 31) // 3 + 1), M_SHYP), (dict(S=1 << 22, n_cand=64), M_SCAND),
       (dict(calm_stride=9), M_STRIDE), (dict(calm_stride=-27), M_STRIDE), (dict(n_total=-1), M_NTOTAL), (dict(n_total=1 << 31), M_NTOTAL),
       (dict(ns_max=-1), M_NSMAX), (dict(ns_max=(1 << 24) + 1), M_NSMAX)] + [({k: None}, M_NULL) for k in OUTPUTS]
# what the forms with a confidence add (the round plan's refusals come after the list above, null `used` after them), and the first failing check stays first
BAD_ROUNDS = [(dict(used=None), M_NULL), (dict(confidence=1.0), M_CONF), (dict(confidence=-0.5), M_CONF), (dict(confidence=float("nan")), M_CONF),
              (dict(first_round=0), M_FIRST), (dict(first_round=6), M_FIRST), (dict(first_round=-4), M_FIRST),
              (dict(confidence=2.0, first_round=6, used=None), M_CONF), (dict(first_round=6, used=None), M_FIRST),
              (dict(S=-1, confidence=2.0), M_S), (dict(n_cand=0, confidence=2.0), M_NCAND), (dict(S=1 << 22, n_cand=64, first_round=6), M_SCAND)]
# ... and the guided forms: the ranking's two arguments before everything else
BAD_GUIDED = [(dict(order=None), M_ORDER), (dict(growth=0), M_GROWTH), (dict(growth=(1 << 31) - (1 << 25) + 1), M_GROWTH),
              (dict(order=None, S=-1), M_ORDER), (dict(growth=0, method=1, confidence=2.0), M_GROWTH)]


@functools.lru_cache(maxsize=None)
def _api():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api


@functools.lru_cache(maxsize=None)
def _synthetic(n, gen_seed):
    """the recipe of tests/test_gpu_robust_scenes.py: 0.5 px noise, a quarter of the matches displaced by U(20, 80) px in views 2 and 3"""
    from tft_vs_fund_amd.scenes import generate_scene_batch
    C, CalM, _, _ = generate_scene_batch(1, n, noise=0.5, seed=gen_seed)
    scene = C[0].copy()
    rng = np.random.default_rng(gen_seed + 100)
    bad = rng.choice(n, n // 4, replace=False)
    scene[bad, 2:6] += rng.uniform(20, 80, size=(bad.size, 4))
    return np.ascontiguousarray(scene), np.ascontiguousarray(CalM)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(a, b, what):
    """two result dicts, bit for bit"""
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.ascontiguousarray(_np(a[k])), np.ascontiguousarray(_np(b[k]))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


# ---- (a) the refusal matrix --------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, rc, text, what):
    assert rc == E_INVALID, (what, rc)
    assert ctx.lib.tff_last_error().decode() == text, (what, ctx.lib.tff_last_error().decode())


@pytest.mark.parametrize("form", ["fixed", "adaptive", "guided", "guided_adaptive"])
def test_refusals_dev(form):
    api = _api()
    ctx = api.Context(0)
    dev = torch.device("cuda", 0)
    scene, CalM = _synthetic(61, 11)
    packed, offsets = api.pack_ragged([scene, scene[:40]])
    canary = 7
    outs = dict(Rt2=torch.empty((2, 12), dtype=torch.float64, device=dev), Rt3=torch.empty((2, 12), dtype=torch.float64, device=dev),
                T=torch.empty((2, 27), dtype=torch.float64, device=dev), mask=torch.empty(101, dtype=torch.uint8, device=dev),
                info=torch.empty((2, 4), dtype=torch.int32, device=dev), status=torch.empty(2, dtype=torch.int32, device=dev),
                used=torch.empty(2, dtype=torch.int32, device=dev))
    base = dict(method=0, scenes=torch.from_numpy(packed).cuda(), offsets=torch.from_numpy(offsets).cuda(), n_total=101, ns_max=61, S=2,
                calm=torch.from_numpy(np.ascontiguousarray(CalM.T).reshape(27)).cuda(), calm_stride=0, seed=1, n_hyp=100, n_sample=0, threshold=4.0, n_cand=4,
                lo_rounds=1, confidence=0.99 if "adaptive" in form else 0.0, first_round=8,
                order=torch.from_numpy(np.concatenate([np.arange(61), np.arange(40)]).astype(np.int32)).cuda(), growth=1000, **outs)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(**kw):
        a = dict(base); a.update(kw)
        head = (ctx.handle, a["method"], p(a["scenes"]), p(a["offsets"]), a["n_total"], a["ns_max"], a["S"], p(a["calm"]), a["calm_stride"], a["seed"],
                a["n_hyp"], a["n_sample"], a["threshold"], a["n_cand"], a["lo_rounds"])
        o = (p(a["Rt2"]), p(a["Rt3"]), p(a["T"]), p(a["mask"]), p(a["info"]))
        if form == "fixed":
            return ctx.lib.tff_robust_pose_scenes_dev(*head, *o, p(a["status"]))
        if form == "adaptive":
            return ctx.lib.tff_robust_pose_scenes_adaptive_dev(*head, a["confidence"], a["first_round"], *o, p(a["used"]), p(a["status"]))
        return ctx.lib.tff_robust_pose_scenes_guided_dev(*head, a["confidence"], a["first_round"], p(a["order"]), a["growth"], *o, p(a["used"]), p(a["status"]))
    assert call() == 0
    torch.cuda.synchronize()
    assert outs["status"].cpu().tolist() == [0, 0]
    for t in outs.values():                                                   # a refused call launches nothing: the outputs keep the canary
        t.fill_(canary)
    torch.cuda.synchronize()
    bad = list(BAD)
    if "adaptive" in form:
        bad += BAD_ROUNDS
    if form == "adaptive":
        bad += [(dict(confidence=0.0), M_CONF)]                               # (0 is a fixed n_hyp for the guided form alone)
    if "guided" in form:
        bad += BAD_GUIDED
    if form == "guided":                                                      # without a confidence neither first_round nor used is looked at
        assert call(first_round=6, used=None) == 0
        torch.cuda.synchronize()
        for t in outs.values():
            t.fill_(canary)
        torch.cuda.synchronize()
    for kw, text in bad:
        _refused(ctx, call(**kw), text, (form, kw))
    ctx.set_rows(0)                                                           # as the ragged call refuses it
    _refused(ctx, call(), M_ROWS, (form, "rows"))
    ctx.set_rows("auto")
    ctx.set_kernel_variant(1)
    _refused(ctx, call(), M_KERNEL, (form, "kernel"))
    ctx.set_kernel_variant(0)
    _refused(ctx, call(S=0, n_cand=0), M_NCAND, (form, "S = 0 is no licence"))
    assert call(S=0) == 0                                                     # an empty list, once the checks have passed: nothing is launched
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == canary).all()), (form, k)
    ctx.close()


@pytest.mark.parametrize("form", ["fixed", "adaptive", "guided", "guided_adaptive"])
def test_refusals_host(form):
    api = _api()
    ctx = api.Context(0)
    scene, CalM = _synthetic(61, 11)
    packed, _ = api.pack_ragged([scene, scene[:40]])
    hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    canary = 7
    h = dict(Rt2=np.empty((2, 12)), Rt3=np.empty((2, 12)), T=np.empty((2, 27)), mask=np.zeros(101, dtype=np.uint8), info=np.zeros((2, 4), dtype=np.int32),
             status=np.zeros(2, dtype=np.int32), used=np.zeros(2, dtype=np.int32))
    calm_h = np.ascontiguousarray(CalM.T).reshape(27)
    order_h = np.concatenate([np.arange(61), np.arange(40)]).astype(np.int32)
    conf = 0.99 if "adaptive" in form else 0.0

    def host(off, S=2, n_cand=4, confidence=conf, first_round=8, order=order_h, growth=1000, used=h["used"]):
        off = None if off is None else np.asarray(off, dtype=np.int64)
        head = (ctx.handle, 0, hp(packed), hp(off), S, hp(calm_h), 0, 1, 100, 0, 4.0, n_cand, 1)
        o = (hp(h["Rt2"]), hp(h["Rt3"]), hp(h["T"]), hp(h["mask"]), hp(h["info"]))
        if form == "fixed":
            return ctx.lib.tff_robust_pose_scenes_host(*head, *o, hp(h["status"]))
        if form == "adaptive":
            return ctx.lib.tff_robust_pose_scenes_adaptive_host(*head, confidence, first_round, *o, hp(used), hp(h["status"]))
        return ctx.lib.tff_robust_pose_scenes_guided_host(*head, confidence, first_round, hp(order), growth, *o, hp(used), hp(h["status"]))
    good = [0, 61, 101]
    assert host(good) == 0 and h["status"].tolist() == [0, 0]
    if form == "guided":
        assert h["used"].tolist() == [100, 100]                               # a fixed n_hyp: used[s] = n_hyp, filled on the host
    for a in h.values():
        a.fill(canary)
    bad = [(dict(off=[0, 61, 40]), M_DECREASING), (dict(off=[-1, 61, 101]), M_NEG_OFF), (dict(off=None), M_NULL_OFF), (dict(off=good, S=-1), M_S),
           (dict(off=[0, (1 << 24) + 1, (1 << 24) + 2]), M_SCENE_BIG), (dict(off=good, n_cand=0), M_NCAND),
           (dict(off=[0, 61, 40], n_cand=0), M_DECREASING)]                   # the offsets before the shared checks
    if "adaptive" in form:
        bad += [(dict(off=good, confidence=1.0), M_CONF), (dict(off=good, first_round=6), M_FIRST), (dict(off=good, used=None), M_NULL),
                (dict(off=[0, 61, 40], confidence=1.0), M_DECREASING)]
    if "guided" in form:
        bad += [(dict(off=good, order=None), M_ORDER), (dict(off=good, growth=0), M_GROWTH), (dict(off=[0, 61, 40], order=None), M_ORDER)]
    for kw, text in bad:
        _refused(ctx, host(**kw), text, (form, kw))
    assert host(good, S=0) == 0
    for k, a in h.items():
        assert (a == canary).all(), (form, k)
    ctx.close()


# ---- (b) one context, one form after another ---------------------------------------------------------------------------------------------------------
def _call_a(ctx):
    api = _api()
    items = [_synthetic(n, 20 + k) for k, n in enumerate((40, 61, 120))]
    packed, off = api.pack_ragged([a for a, _ in items])
    ctx.set_score("count")
    out = ctx.robust_pose_scenes("LinearTFTPoseEstimation", torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(items[0][1]).cuda(),
                                 256, 4.0, seed=5, candidates=4, ns_max=120)
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _call_b(ctx):
    api = _api()
    sizes = (40, 85, 130, 175, 220, 265, 310, 355, 400)
    items = [_synthetic(n, 40 + k) for k, n in enumerate(sizes)]
    packed, off = api.pack_ragged([a for a, _ in items])
    calms = np.stack([c * (1.0 + 0.01 * k) for k, (_, c) in enumerate(items)])   # a CalM per scene
    order = np.concatenate([np.random.default_rng(k).permutation(n) for k, n in enumerate(sizes)]).astype(np.int32)
    ctx.set_score("msac")
    out = ctx.robust_pose_scenes("LinearTFTPoseEstimation", torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(calms).cuda(),
                                 1024, 4.0, seed=9, candidates=16, ns_max=400, confidence=0.99, first_round=64, order=torch.from_numpy(order).cuda(), growth=500)
    torch.cuda.synchronize()
    ctx.set_score("count")
    return {k: _np(v) for k, v in out.items()}


def test_one_context_across_forms():
    api = _api()
    ctx = api.Context(0)
    a1, b, a2 = _call_a(ctx), _call_b(ctx), _call_a(ctx)
    ctx.close()
    assert "n_hyp_used" in b and "score" in b and (a1["status"] == 0).all() and (b["status"] == 0).all()
    _same(a1, a2, "A before and after B")
    for what, got, run in (("A", a1, _call_a), ("B", b, _call_b)):
        fresh = api.Context(0)
        _same(got, run(fresh), what + " on a fresh context")
        fresh.close()


# ---- (c) more candidates than rows in a chunk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [True, False])
def test_more_candidates_than_chunk_rows(adaptive):
    api = _api()
    ctx = api.Context(0)
    method, S, n_hyp, K, seed, thr = "LinearTFTPoseEstimation", 40, 8, 16, 77, 4.0
    items = [_synthetic(40, 60 + s % 4) for s in range(S)]
    scenes = [a for a, _ in items]
    calm = torch.from_numpy(items[0][1]).cuda()
    packed, off = api.pack_ragged(scenes)
    more = dict(confidence=0.9, first_round=4) if adaptive else {}            # C = S * K = 640 candidates; the longest round has S * 4 = 160 rows
    out = ctx.robust_pose_scenes(method, torch.from_numpy(packed).cuda(), torch.from_numpy(off).cuda(), calm, n_hyp, thr, seed=seed, candidates=K,
                                 ns_max=40, **more)
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in out.items()}
    used = out["n_hyp_used"] if adaptive else np.full(S, n_hyp)
    assert set(used.tolist()) <= {4, 8}
    for s in range(S):
        ref = ctx.robust_pose(method, torch.from_numpy(scenes[s]).cuda(), calm, int(used[s]), thr, seed=(seed + s) & MASK64, candidates=K)
        torch.cuda.synchronize()
        one = {k: out[k][s] for k in ("R_t_2", "R_t_3", "T", "inliers", "hypothesis", "refits", "candidates", "status")}
        one["mask"] = out["mask"][off[s]:off[s + 1]]
        _same(one, {k: _np(v) for k, v in ref.items()}, (adaptive, s))
    ctx.close()
