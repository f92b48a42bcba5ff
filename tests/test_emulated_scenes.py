"""
The glue of the many-scenes robust estimator (csrc/robust_scenes_kernel.h) on the lane emulator, no GPU: the kernels are compiled by g++ (tests/emu/emu_scenes.cpp)
and driven with six small scenes (5 .. 130 correspondences), slabs that cut scenes, a launch that starts inside a scene, malformed offsets and a packed
batch smaller than the inliers.  References: api.sample_indices_reference for the sampler, the emulated k_repr_error per scene for the counts, numpy for
offsets, compaction, the winner and the top-K order.  (Bit-identity with the one-scene call on the GPU is tests/test_gpu_robust_scenes.py.)
The one-scene call is this chain with S = 1 and no offsets array (a null SceneSet::offsets = the scene [0, n_total)): the last test drives the sampler, the
count kernel, the flags, offsets + compaction and the finish in that form against the same launch given [0, n] (the k_round_* kernels of the adaptive call
never see null offsets: tests/test_emulated_adaptive.py).
"""
import ctypes
import os
import subprocess

import numpy as np

from tft_vs_fund_amd import api
from tft_vs_fund_amd.scenes import generate_scene_batch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
c_l, c_i, c_d, c_u = ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _lib():
    emu = os.path.join(HERE, "emu")
    csrc = os.path.join(ROOT, "tft_vs_fund_amd", "csrc")
    out_dir = os.path.join(emu, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "libtff_emu_scenes.so")
    deps = [os.path.join(emu, f) for f in ("emu_scenes.cpp", "emu_primitives.h", "hip_emu.h", "wave_target.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-shared", "-fPIC", "-I" + emu, "-I" + csrc, "-o", out,
                        os.path.join(emu, "emu_scenes.cpp")], check=True)
    return ctypes.CDLL(out)


SIZES = [5, 7, 9, 16, 61, 130]
S = len(SIZES)
MASK64 = (1 << 64) - 1


def _synth(n, seed):
    C, CalM, Rt0, _ = generate_scene_batch(1, n, noise=0.5, seed=seed)
    return np.ascontiguousarray(C[0]), np.ascontiguousarray(CalM), Rt0


ITEMS = [_synth(n, 3 + k) for k, n in enumerate(SIZES)]
PACKED, OFF = api.pack_ragged([a for a, _, _ in ITEMS])
CALMS = np.ascontiguousarray(np.stack([c.T.reshape(27) for _, c, _ in ITEMS]))
NTOT = PACKED.shape[0]
BAD_OFF = np.array([0, 5, 4, 21, 37, 98, 300], dtype=np.int64)               # scene 1 decreases, scene 5 ends beyond the packed array


def _set(off, ns_max, n_min):
    return (P(PACKED), P(off), c_l(S), c_l(NTOT), c_i(ns_max), c_i(n_min), P(CALMS), c_l(27))


def _cm(Rt):
    return np.ascontiguousarray(Rt.T).reshape(12)


def _poses(B, first, per, rng):
    """pose b = the ground truth of scene (first + b) // per, two of three perturbed"""
    Rt2 = np.zeros((B, 12)); Rt3 = np.zeros((B, 12))
    for b in range(B):
        Rt0 = ITEMS[(first + b) // per][2]
        e = rng.normal(0, 1e-3 if b % 3 else 0, (2, 3, 4))
        Rt2[b] = _cm(Rt0[0] + e[0]); Rt3[b] = _cm(Rt0[1] + e[1])
    return Rt2, Rt3


def test_sampler_draws_per_scene_with_global_indices():
    L = _lib()
    n, per, seed, first = 7, 37, (1 << 64) - 3, 11                          # the seed wraps at scene 3; the launch starts inside scene 0
    B = S * per - first
    out = np.full((B, n), -7, dtype=np.int32); calm_out = np.zeros((B, 27))
    L.e_sample(*_set(OFF, 130, n), c_u(seed), c_l(first), None, c_l(B), c_l(per), c_i(n), P(out), P(calm_out))
    for b in range(B):
        s, h = divmod(first + b, per)
        if SIZES[s] < n:
            assert (out[b] == -1).all()
        else:
            assert np.array_equal(out[b], api.sample_indices_reference((seed + s) & MASK64, h, 1, n, SIZES[s])[0] + OFF[s]), b
        assert np.array_equal(calm_out[b], CALMS[s])
    K = 3                                                                     # the candidates' form: hypothesis indices from selection keys
    hs = np.random.default_rng(0).integers(0, 1000, S * K)
    keys = np.array([(5 << 32) | (0xFFFFFFFF - int(h)) for h in hs], dtype=np.uint64)
    keys[4] = 0                                                               # no candidate: index 0
    out = np.zeros((S * K, n), dtype=np.int32); calm_out = np.zeros((S * K, 27))
    L.e_sample(*_set(OFF, 130, n), c_u(99), c_l(0), P(keys), c_l(S * K), c_l(K), c_i(n), P(out), P(calm_out))
    for r in range(S * K):
        s = r // K
        if SIZES[s] < n:
            assert (out[r] == -1).all()
        else:
            assert np.array_equal(out[r], api.sample_indices_reference(99 + s, 0 if r == 4 else int(hs[r]), 1, n, SIZES[s])[0] + OFF[s]), r


def test_counts_equal_the_one_scene_kernel_whatever_the_cut():
    """(per_scene, slab, LDS doubles for the scene, first): slabs of one pass and of several, staging for all scenes, for those up to 61, for none"""
    L = _lib()
    rng = np.random.default_rng(1)
    for per, slab, stage, first in ((1, 16, 6 * 130, 0), (3, 16, 6 * 130, 0), (5, 16, 6 * 61, 2), (21, 48, 6 * 130, 0), (21, 32, 0, 7)):
        B = S * per - first
        Rt2, Rt3 = _poses(B, first, per, rng)
        Rt2[1] = np.nan
        for off, ns_max, n_min in ((OFF, 130, 7), (OFF, 61, 0), (BAD_OFF, 130, 0)):
            counts = np.full(B, -9, dtype=np.int32)
            L.e_count(*_set(off, ns_max, n_min), P(Rt2), P(Rt3), c_l(first), c_l(B), c_l(per), c_l(slab), c_d(4.0), P(counts), c_i(stage))
            for s in range(S):
                lo, hi = max(0, s * per - first), (s + 1) * per - first
                if hi <= lo:
                    continue
                o0, o1 = int(off[s]), int(off[s + 1])
                if o0 < 0 or o1 < o0 or o1 > NTOT or o1 - o0 > ns_max or o1 - o0 < n_min:
                    assert (counts[lo:hi] == -1).all(), (per, s)
                    continue
                ref = np.zeros(hi - lo, dtype=np.int32)
                sc = np.ascontiguousarray(PACKED[o0:o1]); r2 = np.ascontiguousarray(Rt2[lo:hi]); r3 = np.ascontiguousarray(Rt3[lo:hi])
                L.e_count_one(P(sc), c_i(o1 - o0), P(np.ascontiguousarray(CALMS[s])), P(r2), P(r3), c_l(hi - lo), c_d(4.0), P(ref))
                assert np.array_equal(counts[lo:hi], ref), (per, slab, stage, first, s)


def test_flags_offsets_compaction_and_winner():
    L = _lib()
    rng = np.random.default_rng(2)
    K = 3; C = S * K
    Rt2 = np.zeros((C, 12)); Rt3 = np.zeros((C, 12))
    for r in range(C):
        Rt0 = ITEMS[r // K][2]; e = rng.normal(0, 1e-3 * (r % K), (2, 3, 4))
        Rt2[r] = _cm(Rt0[0] + e[0]); Rt3[r] = _cm(Rt0[1] + e[1])
    cnt = np.array([10 + r for r in range(C)], dtype=np.int32)
    cnt[4] = -1; cnt[0:3] = -1
    mask = np.full(K * NTOT, 9, dtype=np.uint8); mcnt = np.full(C, -5, dtype=np.int32)
    L.e_mask(*_set(OFF, 130, 7), P(Rt2), P(Rt3), c_l(C), c_l(K), c_d(4.0), P(mask), P(mcnt), P(cnt), None)
    counts = np.zeros(C, dtype=np.int32)
    L.e_count(*_set(OFF, 130, 7), P(Rt2), P(Rt3), c_l(0), c_l(C), c_l(K), c_l(16), c_d(4.0), P(counts), c_i(6 * 130))
    rows = {}
    for r in range(C):
        s, k = divmod(r, K); ns = SIZES[s]
        row = mask[K * OFF[s] + k * ns: K * OFF[s] + (k + 1) * ns]
        if ns < 7 or cnt[r] < 0:                                              # an invalid scene, no such candidate: nothing is written
            assert (row == 9).all() and mcnt[r] == -5, r
            continue
        assert row.max() <= 1 and int(row.sum()) == mcnt[r] == counts[r], r   # the row sums are the count kernel's counts
        rows[r] = row
    offsets = np.full(C + 1, -1, dtype=np.int64); packed_out = np.full((K * NTOT, 6), -1.0)
    pose = rng.normal(size=C * 51); seed_idx = np.arange(C, dtype=np.int32) + 100; nref = np.arange(C, dtype=np.int32) % 3
    o2 = np.zeros((S, 12)); o3 = np.zeros((S, 12)); oT = np.zeros((S, 27)); info = np.zeros((S, 4), dtype=np.int32); status = np.full(S, -1, dtype=np.int32)
    cnt[9:12] = -1                                                            # scene 3: no candidate left
    true = np.concatenate([[0], np.cumsum([int(mcnt[r]) if cnt[r] >= 0 else 0 for r in range(C)])])
    for cap in (K * NTOT, 40):                                                # 40: a packed batch smaller than the inliers -- the offsets stop there
        L.e_cand(*_set(OFF, 130, 7), c_i(K), P(cnt), P(seed_idx), P(nref), P(pose), P(mask), P(mcnt), P(offsets), P(packed_out), c_l(cap),
                 P(o2), P(o3), P(oT), P(info), P(status))
        assert np.array_equal(offsets, np.minimum(true, cap))
        for r in rows:
            if cnt[r] >= 0:
                s = r // K
                got = packed_out[offsets[r]:offsets[r + 1]]
                assert np.array_equal(got, PACKED[OFF[s]:OFF[s + 1]][rows[r] != 0][:got.shape[0]]), r   # in scene order
    assert status.tolist() == [api.ST_TOO_FEW, 0, 0, api.ST_NO_POSE, 0, 0]
    for s in range(S):
        c = cnt[s * K:(s + 1) * K]
        if status[s] != 0:
            assert info[s].tolist() == [0, -1, 0, 0] and np.isnan(o2[s]).all() and np.isnan(o3[s]).all() and np.isnan(oT[s]).all()
            continue
        w = s * K + int(np.argmax(c))                                         # the largest count, ties to the earlier candidate
        assert info[s].tolist() == [int(c.max()), int(seed_idx[w]), int(nref[w]), int((c >= 0).sum())]
        assert np.array_equal(o2[s], pose[w * 12:(w + 1) * 12]) and np.array_equal(o3[s], pose[(C + w) * 12:(C + w + 1) * 12])
        assert np.array_equal(oT[s], pose[C * 24 + w * 27:C * 24 + (w + 1) * 27])


def test_topk_order_with_the_scene_fields():
    L = _lib()
    cn = np.random.default_rng(3).integers(-1, 5, 700).astype(np.int32); sel = np.zeros(5, dtype=np.uint64)
    L.e_topk(P(cn), c_l(700), P(sel), c_i(5), c_i(5), ctypes.c_uint(2))
    order = [h for h in sorted(range(700), key=lambda h: (-cn[h], h)) if cn[h] >= 0][:5]
    assert [0xFFFFFFFF - (int(k) & 0xFFFFFFFF) for k in sel] == order
    assert [(int(k) >> 32) - 1 for k in sel] == [int(cn[h]) for h in order]


def test_null_offsets_are_the_one_scene_zero_to_n_total():
    """scene_range with offsets == null, through every kernel that calls it, against the same launch with the explicit offsets [0, n]: n = 7 (exactly one
    sample), 256 and 257 (the compaction tile), K = 4 with candidates 1 and 2 absent; the sampler also without calm_out (the shared CalM); the count kernel
in place and staged."""
    L = _lib()
    K, n_s, thr = 4, 7, 4.0
    for n in (7, 256, 257):
        scene, CalM, Rt0 = _synth(n, 40 + n)
        calm = np.ascontiguousarray(CalM.T).reshape(27)
        rng = np.random.default_rng(n)

        def both(run):
            """run(offsets) with null and with [0, n]: the two tuples of outputs must be equal array for array"""
            got, ref = run(None), run(np.array([0, n], dtype=np.int64))
            assert len(got) == len(ref)
            for i, (g, r) in enumerate(zip(got, ref)):
                assert np.array_equal(g, r), (n, run.__name__, i)
            return got

        def sset(off):
            return (P(scene), P(off), c_l(1), c_l(n), c_i(n), c_i(n_s), P(calm), c_l(0))

        # the sampler: a chunk of hypotheses (with and without calm_out), then the candidates' form with a key of 0
        def sample(off):
            outs = []
            for with_calm in (True, False):
                out = np.full((50, n_s), -7, dtype=np.int32); calm_out = np.full((50, 27), -3.0)
                L.e_sample(*sset(off), c_u(99), c_l(5), None, c_l(50), c_l(1000), c_i(n_s), P(out), P(calm_out) if with_calm else None)
                outs += [out, calm_out]
            keys = np.array([(5 << 32) | (0xFFFFFFFF - h) for h in (3, 0, 17, 999)], dtype=np.uint64); keys[1] = 0
            out = np.full((K, n_s), -7, dtype=np.int32)
            L.e_sample(*sset(off), c_u(99), c_l(0), P(keys), c_l(K), c_l(K), c_i(n_s), P(out), None)
            return outs + [out]
        idx, copied, idx_alone, untouched, cand_idx = both(sample)
        assert np.array_equal(idx, api.sample_indices_reference(99, 5, 50, n_s, n)) and np.array_equal(idx, idx_alone)
        assert (copied == calm).all() and (untouched == -3.0).all()            # null calm_out: nothing is written
        assert np.array_equal(cand_idx[2], api.sample_indices_reference(99, 17, 1, n_s, n)[0])
        assert np.array_equal(cand_idx[1], api.sample_indices_reference(99, 0, 1, n_s, n)[0])

        # flags of the K candidates, two of them absent
        Rt2 = np.stack([_cm(Rt0[0] + rng.normal(0, 1e-3 * r, (3, 4))) for r in range(K)])
        Rt3 = np.stack([_cm(Rt0[1] + rng.normal(0, 1e-3 * r, (3, 4))) for r in range(K)])
        cnt = np.array([30, -1, -1, 20], dtype=np.int32)

        def flags(off):
            mask = np.full(K * n, 9, dtype=np.uint8); mcnt = np.full(K, -5, dtype=np.int32)
            L.e_mask(*sset(off), P(Rt2), P(Rt3), c_l(K), c_l(K), c_d(thr), P(mask), P(mcnt), P(cnt), None)
            return mask, mcnt
        mask, mcnt = both(flags)
        rows = mask.reshape(K, n)
        assert (rows[1:3] == 9).all() and rows[0].max() <= 1 and int(rows[0].sum()) == mcnt[0] > 0 and int(rows[3].sum()) == mcnt[3]

        # the count kernel: the K rows read in place, sixteen rows (a segment long enough to stage the scene in LDS); its integers are the row sums
        def count(off):
            outs = []
            for rep in (1, 4):
                r2 = np.ascontiguousarray(np.tile(Rt2, (rep, 1))); r3 = np.ascontiguousarray(np.tile(Rt3, (rep, 1))); B = K * rep
                counts = np.full(B, -9, dtype=np.int32)
                L.e_count(*sset(off), P(r2), P(r3), c_l(0), c_l(B), c_l(B), c_l(16), c_d(thr), P(counts), c_i(6 * n))
                outs.append(counts)
            return outs
        c4, c16 = both(count)
        assert c4[0] == mcnt[0] and c4[3] == mcnt[3] and np.array_equal(c16, np.tile(c4, 4))

        # offsets + compaction + the winner
        pose = rng.normal(size=K * 51); seed_idx = np.arange(K, dtype=np.int32) + 100; nref = np.arange(K, dtype=np.int32) % 3

        def cand(off):
            offsets = np.full(K + 1, -1, dtype=np.int64); packed = np.full((K * n, 6), -1.0)
            o2 = np.zeros((1, 12)); o3 = np.zeros((1, 12)); oT = np.zeros((1, 27)); info = np.zeros((1, 4), dtype=np.int32)
            status = np.full(1, -1, dtype=np.int32)
            L.e_cand(*sset(off), c_i(K), P(cnt), P(seed_idx), P(nref), P(pose), P(mask), P(mcnt), P(offsets), P(packed), c_l(K * n),
                     P(o2), P(o3), P(oT), P(info), P(status))
            return offsets, packed, o2, o3, oT, info, status
        offsets, packed, o2, o3, oT, info, status = both(cand)
        assert offsets.tolist() == [0, mcnt[0], mcnt[0], mcnt[0], mcnt[0] + mcnt[3]]
        assert np.array_equal(packed[:offsets[1]], scene[rows[0] != 0]) and np.array_equal(packed[offsets[3]:offsets[4]], scene[rows[3] != 0])
        assert status.tolist() == [0] and info[0].tolist() == [30, 100, 0, 2]
        assert np.array_equal(o2[0], pose[:12]) and np.array_equal(o3[0], pose[K * 12:K * 12 + 12]) and np.array_equal(oT[0], pose[K * 24:K * 24 + 27])
