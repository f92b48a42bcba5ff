"""
The bundle adjustment over tracks on the GPU (tff_bundle_adjust_tracks_batch_dev / _host, include/tftfund_tracks.h; Context.bundle_adjust_views and
api.BundleAdjustment with missing="point") against the numpy restatement (tests/ba_tracks_oracle.py) over every case of tests/ba_tracks_cases.py, at its
gates: status and used exact, iter equal, repr_err, R_t and the Reconst columns of the points taking part within 1e-9 relative, NaN exactly at the dropped
columns.  The cases of one (M, N, Reconst0) go into one batch, one item per visibility pattern.  Bit for bit: an item alone and inside such a batch;
appended all-NaN columns (the padding that serves as the ragged form); the items of a batch in another order.  Against the whole-view call: agreement on
fully visible input, and the difference the feature exists for.
"""
import ctypes
import functools

import numpy as np
import pytest

import ba_tracks_cases as tc
import ba_tracks_oracle as TO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


@functools.lru_cache(maxsize=None)
def _ctx():
    from tft_vs_fund_amd import api
    from tft_vs_fund_amd.build import build_library
    build_library()
    return api.Context(0)


def _dev(cases, missing="point"):
    """cases: [(CalM, R0, C, X0)] of one M, N -> per item (R_t, Reconst, iter, repr_err, used, status)"""
    X0 = np.stack([c[3] for c in cases]) if cases[0][3] is not None else None
    out = _ctx().bundle_adjust_views(cases[0][0], np.stack([c[1] for c in cases]), np.stack([np.ascontiguousarray(c[2].T) for c in cases]), X0, missing=missing)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    used = o["used"] if missing == "point" else np.full(len(cases), -1)
    return [(o["R_t"][b], o["Reconst"][b], int(o["iter"][b]), float(o["repr_err"][b]), int(used[b]), int(o["status"][b])) for b in range(len(cases))]


def _host(cases):
    ctx = _ctx()
    B = len(cases); M, N = cases[0][2].shape[0] // 2, cases[0][2].shape[1]
    calm = np.ascontiguousarray(cases[0][0].T).reshape(-1)
    rt = np.stack([np.ascontiguousarray(c[1].T).reshape(-1) for c in cases]); Cc = np.stack([np.ascontiguousarray(c[2].T) for c in cases])
    x0 = np.stack([np.ascontiguousarray(c[3].T) for c in cases]) if cases[0][3] is not None else None
    o = np.full((B, 12 * M), 5.0); rec = np.full((B, N, 3), 5.0); it = np.full(B, 5, dtype=np.int32); err = np.full(B, 5.0)
    used = np.full(B, -5, dtype=np.int32); st = np.full(B, 5, dtype=np.int32)
    assert ctx.lib.tff_bundle_adjust_tracks_batch_host(ctx.handle, M, P(calm), 0, P(rt), P(Cc), B, N, P(x0), P(o), P(rec), P(it), P(err), P(used), P(st)) == 0
    return [(o[b].reshape(4, 3 * M).T, rec[b].T, int(it[b]), float(err[b]), int(used[b]), int(st[b])) for b in range(B)]


def _biteq(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


GROUPS = [(M, N, x0) for M in tc.VIEWS for N in tc.SIZES for x0 in (False, True)]


@pytest.mark.parametrize("M,N,with_x0", GROUPS)
def test_every_case_matches_the_restatement_dev_and_host(M, N, with_x0):
    pats = [p for p in tc.PATTERNS if tc.applicable(M, N, p)]
    cases = [tc.synthetic(M, N, p, with_x0) for p in pats]
    dev, host = _dev(cases), _host(cases)
    for p, d, h in zip(pats, dev, host):
        ref = tc.reference("syn", M, N, p, with_x0)
        tc.gate(d, ref, (M, N, p, with_x0, "dev"))
        tc.gate(h, ref, (M, N, p, with_x0, "host"))
        assert _biteq(d, h), (M, N, p, with_x0)                              # the same kernel on the same bytes


@pytest.mark.parametrize("dataset,first,M,n_tracks", tc.REAL)
def test_epfl_windows_match_the_restatement(dataset, first, M, n_tracks):
    case = tc.real(dataset, first, M, n_tracks)
    ref = tc.reference("real", dataset, first, M, n_tracks)
    tc.gate(_dev([case])[0], ref, (dataset, first, M, "dev"))
    tc.gate(_host([case])[0], ref, (dataset, first, M, "host"))


def test_failing_items_inside_a_batch_of_good_ones():
    good = tc.synthetic(3, 12, "random", False)
    for kind in tc.FAILING:
        case, used, status = tc.failing(kind)
        if case[3] is not None:
            batch = [tc.synthetic(3, 12, "random", True), case, tc.synthetic(3, 12, "full", True)]
            refs = [tc.reference("syn", 3, 12, "random", True), tc.reference("fail", kind), tc.reference("syn", 3, 12, "full", True)]
        else:
            batch = [good, case, tc.synthetic(3, 12, "full", False)]
            refs = [tc.reference("syn", 3, 12, "random", False), tc.reference("fail", kind), tc.reference("syn", 3, 12, "full", False)]
        assert (refs[1][4], refs[1][5]) == (used, status)
        for run in (_dev, _host):
            for got, ref in zip(run(batch), refs):
                tc.gate(got, ref, (kind, run.__name__))
    from tft_vs_fund_amd import api
    with pytest.raises(ValueError):
        api.BundleAdjustment(*tc.failing("too_few")[0], missing="point")
    with pytest.raises(ValueError):
        api.BundleAdjustment(*tc.failing("single")[0], missing="point")


@pytest.mark.parametrize("M,N", [(3, 65), (6, 130), (2, 64)])
def test_an_item_alone_equals_the_item_in_a_batch_in_any_order(M, N):
    """one wavefront per problem: an item's outputs are the same alone (B = 1), inside a batch of items with other visibility patterns, and when the
    patterns are permuted among the items of the batch"""
    pats = [p for p in tc.PATTERNS if tc.applicable(M, N, p)]
    cases = [tc.synthetic(M, N, p, False) for p in pats]
    batch = _dev(cases)
    for p, c, b in zip(pats, cases, batch):
        assert _biteq(_dev([c])[0], b), (M, N, p)
    perm = np.random.default_rng(5).permutation(len(cases))
    shuffled = _dev([cases[k] for k in perm])
    for n, k in enumerate(perm):
        assert _biteq(shuffled[n], batch[k]), (M, N, pats[k])
    rolled = _dev(cases[1:] + cases[:1])                                     # every pattern on its neighbour's place
    for n in range(len(cases)):
        assert _biteq(rolled[n], batch[(n + 1) % len(cases)]), (M, N, n)


@pytest.mark.parametrize("N0,N1", [(64, 65), (65, 130)])
def test_appended_nan_columns_change_no_bit(N0, N1):
    """Appending all-NaN columns changes no bit of R_t, iter, repr_err, used, nor of the other Reconst columns: problems of different N go into one
    batch padded with NaN columns -- here N0 and N1 in ONE call, against each alone."""
    for M, pattern, with_x0 in ((3, "random", False), (4, "one_missing", True), (6, "few_obs", True), (6, "full", False)):
        small = tc.synthetic(M, N0, pattern, with_x0)
        big = tc.synthetic(M, N1, "random" if M > 2 else "full", with_x0)
        pad = np.full((2 * M, N1 - N0), np.nan)
        padded = (small[0], small[1], np.hstack([small[2], pad]), np.hstack([small[3], np.full((3, N1 - N0), 7.0)]) if with_x0 else None)
        a = _dev([small])[0]
        both = _dev([padded, big])
        b = both[0]
        assert a[2:] == b[2:] and a[0].tobytes() == b[0].tobytes(), (M, pattern)
        assert np.ascontiguousarray(a[1]).tobytes() == np.ascontiguousarray(b[1][:, :N0]).tobytes() and np.isnan(b[1][:, N0:]).all(), (M, pattern)
        assert _biteq(both[1], _dev([big])[0])
        tc.gate(b[:1] + (b[1][:, :N0],) + b[2:], tc.reference("syn", M, N0, pattern, with_x0), (M, N0, pattern, "padded"))


def test_against_the_whole_view_call(capsys):
    """Fully visible input: missing="point" agrees with missing="view" at the gates, with the same iter (whether the bits agree is printed, not
    asserted).  One view missing from one point: the whole-view call leaves that camera at its start, this one moves it."""
    same_bits = []
    for M, N, with_x0 in ((2, 12, False), (3, 65, True), (4, 64, False), (6, 130, True)):
        case = tc.synthetic(M, N, "full", with_x0)
        pt, vw = _dev([case])[0], _dev([case], missing="view")[0]
        tc.gate(pt, tc.reference("syn", M, N, "full", with_x0), (M, N, "point"))
        tc.gate(vw[:4] + (N, vw[5]), tc.reference("syn", M, N, "full", with_x0), (M, N, "view"))
        assert pt[2] == vw[2]
        same_bits.append(((M, N, with_x0), _biteq(pt[:4], vw[:4])))
    with capsys.disabled():
        print("\nmissing=point vs missing=view on fully visible input, bits equal:", same_bits)
    M, N = 4, 65
    CalM, R0, C, X0 = tc.synthetic(M, N, "one_missing", False)
    pt, vw = _dev([(CalM, R0, C, X0)])[0], _dev([(CalM, R0, C, X0)], missing="view")[0]
    G = np.vstack([R0[0:3], [0, 0, 0, 1]])
    start = R0[3:6] @ np.linalg.inv(G)                                       # camera 2 in the frame of camera 1 (:80-86)
    assert vw[5] == 0 and np.abs(vw[0][3:6, :3] - start[:, :3]).max() < 1e-12        # the whole-view call: view 2 dropped, its camera where it started
    assert pt[5] == 0 and pt[4] == N and np.abs(pt[0][3:6, :3] - start[:, :3]).max() > 1e-4      # this call: adjusted (the start is ~0.5 degrees off)
    full = tc.reference("syn", M, N, "full", False)
    assert np.abs(pt[0] - full[0]).max() < 1e-3                              # ... to nearly where all N observations of that view put it
    from tft_vs_fund_amd import api
    R_t, Rec, it, err = api.BundleAdjustment(CalM, R0, C, None, missing="point")
    assert it == pt[2] and R_t.tobytes() == np.ascontiguousarray(pt[0]).tobytes() and err == pt[3]
