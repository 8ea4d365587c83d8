"""A small mock of what loopClosing::SearchMatch reads (a current keyframe, loop candidates, text objects with their observations, the matched map texts), the
file tests/cxx/loop_match_from_cxx.cpp reads it from, and the bytes that driver has to write: the same gathering as adapter/tsorb_loop_match.hpp, done
here in Python over the Python mirror (ORBextractor.match_brute_text / match_brute_scene).

in.bin (little endian; i32 unless said):
  w, h, n_kf (keyframe 0 = the current one, the others the candidates), n_obj
  per keyframe: n_keys; xy f32 [n_keys][2]; desc u8 [n_keys][32]; vTextObjInfo [n_keys]; vMatches2D3D [n_keys]; n_dete; vTextDeteCorMap [n_dete];
                per detection: corners f64 [4][2]; rows (= vKeysText[i].size() = mDescrText[i].rows); u8 [rows][32]
  per object:   n_obs; per observation: keyframe, n_idx, idx [n_idx]                    (mapText::GetObvIdx)
  n_obv; per observation of the current keyframe (vObvText): object, n_idx, idx [n_idx]
  per observation of the current keyframe: n_res; object [n_res]                         (vMatchTexts)
out.bin: per candidate: n_pair; per pair: iObvText, iMatchRes, idxCur, idxCan, n_good, n_good x (queryIdx i32, trainIdx i32, distance f32);
                        n_box; quad_cur f64 [n_box][8]; quad_can f64 [n_box][8]; n1; vMatchIdx12 [n1]; nMatches"""
import struct
import numpy as np


def _flip(rng, row, nbits):
    row = row.copy()
    for b in rng.choice(256, nbits, replace=False):
        row[b >> 3] ^= np.uint8(1 << (b & 7))
    return row


def make_world(seed, w=320, h=240, n_cand=3, n_obj=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (160, 32), dtype=np.uint8)
    obj_desc = [rng.integers(0, 256, (int(rng.integers(8, 40)), 32), dtype=np.uint8) for _ in range(n_obj)]
    kfs = []
    for k in range(1 + n_cand):
        n = 160 if k == 0 else int(rng.integers(120, 200))
        src = rng.integers(0, 160, n) if k else np.arange(160)
        desc = np.stack([_flip(rng, base[s], int(rng.integers(0, 45))) for s in src])
        n_dete = n_obj
        dete, tdesc = [], []
        for d in range(n_dete):
            cx, cy = rng.uniform(40, w - 40), rng.uniform(30, h - 30)
            hw, hh = rng.uniform(10, 30), rng.uniform(6, 16)
            dete.append(np.array([[cx - hw, cy - hh], [cx + hw, cy - hh], [cx + hw, cy + hh], [cx - hw, cy + hh]]) + rng.uniform(-4, 4, (4, 2)))
            rows = obj_desc[d][rng.permutation(len(obj_desc[d]))[:int(rng.integers(5, len(obj_desc[d]) + 1))]]
            tdesc.append(np.stack([_flip(rng, r, int(rng.integers(0, 40))) for r in rows]))
        if k == 2:
            tdesc[1] = tdesc[1][:1]                                    # a detection with a single text keypoint: the pair is skipped (loopClosing.cc:799)
        info = np.where(rng.uniform(size=n) < 0.25, rng.integers(0, n_dete, n), -1).astype(np.int32)
        kfs.append(dict(xy=np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32), desc=desc, info=info,
                        m2d3d=np.where(rng.uniform(size=n) < 0.8, rng.integers(0, 500, n), -1).astype(np.int32),
                        cormap=np.where(rng.uniform(size=n_dete) < 0.8, np.arange(n_dete), -1).astype(np.int32), dete=dete, tdesc=tdesc))
    objs = []                                                          # object d is seen as detection d wherever it is seen
    for d in range(n_obj):
        obs = []
        for k in range(1 + n_cand):
            if d == 3 and k == 1:
                continue                                               # candidate 1 does not observe object 3
            obs.append((k, [] if (d == 4 and k == 3) else [d]))        # candidate 3's observation of object 4 has no detection index
        objs.append(obs)
    obv = [(d, [d] if d != 2 else []) for d in range(n_obj)]           # the current keyframe's observation of object 2 has no detection index
    res = [[d, (d + 1) % n_obj] if d != 1 else [] for d in range(n_obj)]   # two matched map texts per observation, none for observation 1
    return dict(w=w, h=h, kfs=kfs, objs=objs, obv=obv, res=res)


def write_world(path, W):
    i32 = lambda *v: struct.pack("<%di" % len(v), *[int(x) for x in v])
    with open(path, "wb") as f:
        f.write(i32(W["w"], W["h"], len(W["kfs"]), len(W["objs"])))
        for K in W["kfs"]:
            n = len(K["xy"])
            f.write(i32(n)); f.write(K["xy"].astype("<f4").tobytes()); f.write(K["desc"].tobytes()); f.write(K["info"].astype("<i4").tobytes()); f.write(K["m2d3d"].astype("<i4").tobytes())
            f.write(i32(len(K["dete"]))); f.write(K["cormap"].astype("<i4").tobytes())
            for q, t in zip(K["dete"], K["tdesc"]):
                f.write(np.ascontiguousarray(q, "<f8").tobytes()); f.write(i32(len(t))); f.write(np.ascontiguousarray(t, np.uint8).tobytes())
        for obs in W["objs"]:
            f.write(i32(len(obs)))
            for k, idx in obs:
                f.write(i32(k, len(idx), *idx))
        f.write(i32(len(W["obv"])))
        for d, idx in W["obv"]:
            f.write(i32(d, len(idx), *idx))
        for r in W["res"]:
            f.write(i32(len(r), *r))


def _has3d(K):
    return np.array([(K["m2d3d"][i] >= 0) if K["info"][i] < 0 else (K["cormap"][K["info"][i]] >= 0) for i in range(len(K["info"]))], np.uint8)


def expected_bytes(W, ex):
    cur, cands = W["kfs"][0], W["kfs"][1:]
    per_cand, pairs = [], []
    for ic in range(len(cands)):
        mine = []
        for i_obv, (obj, idx_cur) in enumerate(W["obv"]):
            if not idx_cur:
                continue
            for i_res, mobj in enumerate(W["res"][i_obv]):
                seen = [idx for k, idx in W["objs"][mobj] if k == ic + 1]
                if not seen or not seen[0]:
                    continue
                idx_can = seen[0][0]
                if len(cands[ic]["tdesc"][idx_can]) <= 1:
                    continue
                mine.append((i_obv, i_res, idx_cur[0], idx_can))
                pairs.append((cur["tdesc"][idx_cur[0]], cands[ic]["tdesc"][idx_can]))
        per_cand.append(mine)
    text = ex.match_brute_text(pairs)
    scene_cands = [dict(xy=K["xy"], desc=K["desc"], has3d=_has3d(K),
                        quad_cur=np.array([cur["dete"][p[2]] for p in per_cand[ic]]).reshape(-1, 4, 2),
                        quad_can=np.array([K["dete"][p[3]] for p in per_cand[ic]]).reshape(-1, 4, 2)) for ic, K in enumerate(cands)]
    m12, nm = ex.match_brute_scene(W["w"], W["h"], cur["xy"], cur["desc"], _has3d(cur), scene_cands)
    out, p = b"", 0
    for ic, mine in enumerate(per_cand):
        out += struct.pack("<i", len(mine))
        for (i_obv, i_res, a, b) in mine:
            t = text[p]; p += 1
            g = np.flatnonzero(t["good"])
            out += struct.pack("<5i", i_obv, i_res, a, b, len(g))
            for q in g:
                out += struct.pack("<iif", int(q), int(t["train_idx"][q]), float(t["dist"][q]))
        out += struct.pack("<i", len(mine))
        out += np.ascontiguousarray(scene_cands[ic]["quad_cur"], "<f8").tobytes() + np.ascontiguousarray(scene_cands[ic]["quad_can"], "<f8").tobytes()
        out += struct.pack("<i", m12.shape[1]) + m12[ic].astype("<i4").tobytes() + struct.pack("<i", int(nm[ic]))
    return out
