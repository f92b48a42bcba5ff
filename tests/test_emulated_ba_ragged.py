"""
The launch plan of the ragged, masked BundleAdjustment (csrc/ba_ragged_kernel.h) around the unchanged k_bundle_adjust, on the lane emulator, no GPU:
count, scan, classes, compact, the three class launches and the scatter, compiled by g++ (tests/emu/emu_ba_ragged.cpp) and run with the class bounds
(8, 20, 64) on items of 1, 7, 8, 9, 20, 21, 63, 64, 65 selected matches; masks that are random (~70 %), all ones, a single survivor, all zero, or
absent; a decreasing offset and one above n_total.  References: numpy for the plan, the emulated fixed-N kernel on the selected matches (bit for bit),
oracle.ba_oracle.BundleAdjustment for three items (1e-9 and the same `iter`, the tolerance of tests/test_bundle_adjustment.py).
(Bit-identity with the fixed-N entry point on the GPU is tests/test_gpu_ba_ragged.py.)
"""
import ctypes
import os
import subprocess

import numpy as np

from oracle import ba_oracle as BA
from tft_vs_fund_amd import api
from tft_vs_fund_amd.scenes import generate_scene_batch, scene_cameras

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i = ctypes.c_long, ctypes.c_int
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
BOUNDS = np.array([8, 20, 64], dtype=np.int32)
COUNTS = [63, 1, 7, 8, 9, 20, 21, 64, 65]                                   # (item 0 is of the last class: in no class list is slot == item)


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_ba_ragged.so")
    deps = [os.path.join(emu, f) for f in ("emu_ba_ragged.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_ba_ragged.cpp")], check=True)
    return ctypes.CDLL(out)


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def _item(n, seed, focalL):
    """n noisy correspondences, their CalM (every item its own focal length, so its own CalM), start poses near the truth (|t2| = 1 scale, ~0.5 degrees /
    1 % off) and start points"""
    rng = np.random.default_rng(100 + seed)
    C, CalM, Rt0, X = generate_scene_batch(1, n, noise=0.5, seed=seed, focalL=focalL)
    sc = np.linalg.norm(Rt0[0][:, 3])
    start = []
    for Rt in Rt0:
        w = 0.01 * rng.standard_normal(3); th = np.linalg.norm(w); k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx) @ Rt[:, :3]
        start.append(np.hstack([R, (Rt[:, 3:4] / sc) * (1 + 0.01 * rng.standard_normal((3, 1)))]))
    K, Ps, _, _ = scene_cameras(focalL)
    M1 = np.linalg.solve(K, Ps[0]); M1 = M1 / np.linalg.norm(M1[0, :3])         # [R1 | -R1 C1]: the points in the frame of camera 1
    X0 = (X[0] @ M1[:, :3].T + M1[:, 3]) / sc * (1 + 0.01 * rng.standard_normal((n, 3)))
    return np.ascontiguousarray(C[0]), CalM, start, np.ascontiguousarray(X0)


class Batch:
    def __init__(self, sizes, seed0):
        items = [_item(n, seed0 + k, 38.0 + 3.0 * k) for k, n in enumerate(sizes)]
        self.items = items
        assert all(not np.array_equal(items[0][1], it[1]) for it in items[1:])   # a CalM per item: an item read with another one's calibration shows
        self.packed, self.off = api.pack_ragged([it[0] for it in items])
        self.calms = np.ascontiguousarray(np.stack([it[1].T.reshape(27) for it in items]))
        self.r2 = np.ascontiguousarray(np.stack([_cm(it[2][0]) for it in items]))
        self.r3 = np.ascontiguousarray(np.stack([_cm(it[2][1]) for it in items]))
        self.x0 = np.ascontiguousarray(np.concatenate([it[3] for it in items]))
        self.B = len(sizes)
        self.ntot = self.packed.shape[0]


def _run(L, bt, off, mask, with_x0, with_rec=True):
    B, nt = bt.B, bt.ntot
    w = dict(m=np.full(B, -7, dtype=np.int32), coff=np.full(B, -7, dtype=np.int64), cls_count=np.full(3, -7, dtype=np.int32),
             cls_list=np.full(3 * B, -7, dtype=np.int32), packed=np.full((nt, 6), -1.0), rec0=np.full((nt, 3), -1.0), src=np.full(nt, -7, dtype=np.int32),
             rec_ws=np.full((nt, 3), -1.0), Rt2=np.full((B, 12), 5.0), Rt3=np.full((B, 12), 5.0), reconst=np.full((nt, 3), 5.0) if with_rec else None,
             iter=np.full(B, -7, dtype=np.int32), repr_err=np.full(B, 5.0), used=np.full(B, -7, dtype=np.int32), status=np.full(B, -7, dtype=np.int32))
    L.e_ba_ragged(P(bt.packed), P(off), c_l(B), c_l(nt), P(mask), P(bt.calms), c_l(27), P(bt.r2), P(bt.r3), P(bt.x0 if with_x0 else None), P(BOUNDS),
                  P(w["m"]), P(w["coff"]), P(w["cls_count"]), P(w["cls_list"]), P(w["packed"]), P(w["rec0"]), P(w["src"]), P(w["rec_ws"]),
                  P(w["Rt2"]), P(w["Rt3"]), P(w["reconst"]), P(w["iter"]), P(w["repr_err"]), P(w["used"]), P(w["status"]))
    return w


def _fixed(L, bt, off, b, sel, with_x0):
    """the emulated fixed-N kernel on item b's selected matches alone"""
    C = np.ascontiguousarray(bt.packed[off[b]:off[b + 1]][sel]); N = C.shape[0]
    x0 = np.ascontiguousarray(bt.x0[off[b]:off[b + 1]][sel]) if with_x0 else None
    o = dict(Rt2=np.zeros(12), Rt3=np.zeros(12), rec=np.zeros((N, 3)), iter=np.zeros(1, dtype=np.int32), err=np.zeros(1), st=np.zeros(1, dtype=np.int32))
    L.e_ba_fixed(P(np.ascontiguousarray(bt.calms[b])), c_l(0), P(np.ascontiguousarray(bt.r2[b])), P(np.ascontiguousarray(bt.r3[b])), P(C), c_l(1), c_i(N), P(x0),
                 P(o["Rt2"]), P(o["Rt3"]), P(o["rec"]), P(o["iter"]), P(o["err"]), P(o["st"]))
    return o


def _biteq(a, b):
    """bit for bit, NaNs included"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _expected_status(off, b, ntot, sel_count):
    o0, o1 = int(off[b]), int(off[b + 1])
    if o0 < 0 or o1 < o0 or o1 > ntot:
        return api.ST_BAD_OFFSETS
    if sel_count == 0:
        return api.ST_TOO_FEW
    return api.ST_TOO_LARGE if sel_count > BOUNDS[2] else 0


def _check(L, bt, off, mask, with_x0, w, oracle_items=(), shared_rec=()):
    """shared_rec: items whose ranges overlap another item's (malformed offsets): they race for those positions of reconst, which are not compared"""
    B, nt = bt.B, bt.ntot
    sels, st = [], []
    for b in range(B):
        o0, o1 = int(off[b]), int(off[b + 1])
        ok = 0 <= o0 <= o1 <= nt
        sel = (mask[o0:o1] != 0 if mask is not None else np.ones(o1 - o0, dtype=bool)) if ok else np.zeros(0, dtype=bool)
        sels.append(sel); st.append(_expected_status(off, b, nt, int(sel.sum())))
    m = np.array([int(s.sum()) if e == 0 else 0 for s, e in zip(sels, st)], dtype=np.int32)
    # the plan against its numpy statement
    assert np.array_equal(w["m"], m) and np.array_equal(w["used"], m)
    cls = np.where(m <= 0, -1, np.where(m <= BOUNDS[0], 0, np.where(m <= BOUNDS[1], 1, 2)))
    assert w["cls_count"].tolist() == [int((cls == c).sum()) for c in range(3)]
    for c in range(3):
        assert sorted(w["cls_list"][c * B:c * B + w["cls_count"][c]].tolist()) == np.nonzero(cls == c)[0].tolist()
    if mask is not None:
        coff = np.concatenate([[0], np.cumsum(m)])[:B]
        assert np.array_equal(w["coff"], coff)
        for b in range(B):
            if m[b] > 0:
                o0, o1 = int(off[b]), int(off[b + 1])
                assert np.array_equal(w["packed"][coff[b]:coff[b] + m[b]], bt.packed[o0:o1][sels[b]]), b       # in scene order
                assert np.array_equal(w["src"][coff[b]:coff[b] + m[b]], np.nonzero(sels[b])[0]), b
                if with_x0:
                    assert np.array_equal(w["rec0"][coff[b]:coff[b] + m[b]], bt.x0[o0:o1][sels[b]]), b
        assert (w["packed"][int(m.sum()):] == -1.0).all() and (w["src"][int(m.sum()):] == -7).all()             # nothing beyond the selected slots
    # every item against the emulated fixed-N kernel on its selected matches, bit for bit
    touched = np.zeros(nt, dtype=bool)
    for b in range(B):
        o0, o1 = int(off[b]), int(off[b + 1])
        if st[b] != 0:
            assert w["status"][b] == st[b] and w["iter"][b] == 0 and np.isnan(w["repr_err"][b]) and np.isnan(w["Rt2"][b]).all() and np.isnan(w["Rt3"][b]).all(), b
            if st[b] != api.ST_BAD_OFFSETS:
                assert np.isnan(w["reconst"][o0:o1]).all(), b
                touched[o0:o1] = True
            continue
        ref = _fixed(L, bt, off, b, sels[b], with_x0)
        assert w["status"][b] == ref["st"][0] and w["iter"][b] == ref["iter"][0], b
        assert _biteq(w["repr_err"][b:b + 1], ref["err"]) and _biteq(w["Rt2"][b], ref["Rt2"]) and _biteq(w["Rt3"][b], ref["Rt3"]), b
        rec = w["reconst"][o0:o1]
        touched[o0:o1] = True
        if b in shared_rec:
            continue
        assert _biteq(rec[sels[b]], ref["rec"]) and np.isnan(rec[~sels[b]]).all(), b
        if b in oracle_items:
            it = bt.items[b]
            R_t_0 = np.vstack([np.eye(3, 4), it[2][0], it[2][1]])
            Ro, Xo, ito, erro = BA.BundleAdjustment(it[1], R_t_0, it[0][sels[b]].T.copy(), it[3][sels[b]].T.copy() if with_x0 else None)
            assert ref["st"][0] == 0 and w["iter"][b] == ito and abs(w["repr_err"][b] - erro) <= 1e-9 * erro
            rel = lambda a, r: np.abs(a - r).max() / np.abs(r).max()
            assert rel(w["Rt2"][b].reshape(4, 3).T, Ro[3:6]) < 1e-9 and rel(w["Rt3"][b].reshape(4, 3).T, Ro[6:9]) < 1e-9 and rel(rec[sels[b]].T, Xo) < 1e-9
    assert (w["reconst"][~touched] == 5.0).all()                                                               # a malformed item's range is left alone
    return st


def _random_mask(sizes, keep, rng):
    """exactly keep[b] flags set in item b (255 now and then: any non-zero byte selects)"""
    parts = []
    for n, k in zip(sizes, keep):
        row = np.zeros(n, dtype=np.uint8)
        row[rng.choice(n, k, replace=False)] = rng.choice([1, 255], k)
        parts.append(row)
    return np.concatenate(parts)


def test_random_masks_with_start_points():
    """~70 % kept, the selected counts exact; a single survivor (the item of 1) and an all-zero item; reconst0 given; three items (63, 20, 21 matches)
    against the oracle"""
    L = _lib()
    rng = np.random.default_rng(7)
    keep = COUNTS + [0]
    sizes = [int(np.ceil(k / 0.7)) if k > 1 else 12 for k in COUNTS] + [10]
    bt = Batch(sizes, 20)
    mask = _random_mask(sizes, keep, rng)
    w = _run(L, bt, bt.off, mask, True)
    st = _check(L, bt, bt.off, mask, True, w, oracle_items=(0, 5, 6))
    assert st == [0] * 8 + [api.ST_TOO_LARGE, api.ST_TOO_FEW]


def test_no_mask_and_malformed_offsets():
    """mask NULL: the kernel reads the caller's arrays; the points are triangulated; item 3 ends before it starts, item 9 ends beyond n_total"""
    L = _lib()
    bt = Batch(COUNTS + [6], 40)
    w = _run(L, bt, bt.off, None, False)
    st = _check(L, bt, bt.off, None, False, w)
    assert st == [0] * 8 + [api.ST_TOO_LARGE, 0]
    bad = bt.off.copy()
    bad[4] = bad[3] - 2                                                       # item 3 decreases; item 4 starts inside item 2
    bad[10] = bt.ntot + 3
    w2 = _run(L, bt, bad, None, False)
    st2 = _check(L, bt, bad, None, False, w2, shared_rec=(2, 4))
    assert st2[3] == api.ST_BAD_OFFSETS and st2[9] == api.ST_BAD_OFFSETS and st2[0] == 0
    for b in (0, 1, 2, 5, 6, 7):                                              # the neighbours are those of the clean run
        assert _biteq(w2["Rt2"][b], w["Rt2"][b]) and w2["iter"][b] == w["iter"][b]


def test_all_ones_mask_and_overlap_overflow():
    """an all-ones mask gives the bits of the call without one; ranges that overlap (malformed offsets) and select more than n_total in all: the item
    that would overrun the compact arrays is ST_BAD_OFFSETS and nothing is written beyond them"""
    L = _lib()
    sizes = [7, 9, 21, 64, 5]
    bt = Batch(sizes, 60)
    ones = np.ones(bt.ntot, dtype=np.uint8)
    w = _run(L, bt, bt.off, ones, False)
    _check(L, bt, bt.off, ones, False, w)
    w0 = _run(L, bt, bt.off, None, False)
    for k in ("Rt2", "Rt3", "reconst", "repr_err"):
        assert _biteq(w[k], w0[k]), k
    for k in ("iter", "status", "used"):
        assert np.array_equal(w[k], w0[k]), k
    over = np.array([0, 60, 0, 60, 0, 60], dtype=np.int64)                    # items 0, 2, 4 all own [0, 60): 180 selected of 106; items 1, 3 decrease
    w = _run(L, bt, over, ones, False, with_rec=False)
    assert w["status"].tolist() == [0] + [api.ST_BAD_OFFSETS] * 4
    assert w["used"].tolist() == [60, 0, 0, 0, 0] and np.isnan(w["Rt2"][1:]).all() and not np.isnan(w["Rt2"][0]).any()
    assert (w["packed"][60:] == -1.0).all() and (w["src"][60:] == -7).all()
