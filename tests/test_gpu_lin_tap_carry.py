"""The text lanes of k_linearize project every photometric tap ONCE (tsba_kernels_lin.h, lin_body): the fetch loop parks what its projection produced -- (mx, my),
1/s, 1/z, u, v -- in the wave's transpose area and the evaluation loop rebuilds the rest (Rm, Pm, P) from it with tap_project's own expressions; the taps' offsets
are immediates instead of lane-indexed loads from the constant tables.  The partner (tsba_debug_options.trial_launches = 4, lin_body<.., REDO>) keeps the evaluation
that projects every tap a second time.  The carried values are what the second projection computes, so the two must agree bit for bit: the reduced system of
the first linearisation (S, g, cost) and a whole solve (parameters, flags, costs, iteration counts)."""
import os
import sys
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEATS = (70, 33, 7)          # level 0: two chunks of 64 features per plane; no count is a multiple of 64 or of 8, two are odd
REPORT_FIELDS = ("iters", "accepted", "termination", "cost0", "cost1", "n_sblock", "n_tblock", "n_bad_scene", "n_bad_tfeat", "n_bad_text")
PARAMS = ("pose", "rho", "theta", "sgood", "tobs_good", "tfgood")
_problems = {}


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


def _tap_sides(P, text):
    """Which sides of the image the level-0 taps of plane `text` fall off in the keyframes that observe it: (left, right, top, bottom, inside) counts."""
    h, w = P.img[0][0].shape[-2:]
    n = np.zeros(5, np.int64)
    for t in range(P.n_tobs):
        if int(P.tobs_text[t]) != text:
            continue
        for f in range(int(P.tfeat_off[0][text]), int(P.tfeat_off[0][text + 1])):
            uv = synth.text_tap_uv(P, 0, int(P.tobs_kf[t]), text, P.tfeat_uv[0][f])
            u, v = uv[:, 0], uv[:, 1]
            out = (np.floor(u) < 0, np.ceil(u) >= w, np.floor(v) < 0, np.ceil(v) >= h)
            for k in range(4):
                n[k] += int(out[k].sum())
            n[4] += int((~(out[0] | out[1] | out[2] | out[3])).sum())
    return n


def _problem(name):
    if name in _problems:
        return _problems[name]
    if name == "golden":
        sys.path.insert(0, GOLD)
        import make_golden
        P, _ = make_golden.make_case("tiny_local")
    elif name == "frozen":                                      # (every text host outside the window: pair_from_Twr)
        P = synth.make_problem(n_kf=5, n_pt=200, n_text=4, feats=FEATS, frozen_frac=1.0)
        assert np.all(P.text_host < 0)
    elif name == "hosted":                                      # (every text host a keyframe of the window: pair_from_poses)
        P = synth.make_problem(n_kf=5, n_pt=200, n_text=4, feats=FEATS, frozen_frac=0.0)
        assert np.all(P.text_host >= 0)
    else:
        P = synth.make_problem(n_kf=5, n_pt=200, n_text=4, feats=FEATS)
        assert int(P.tfeat_off[0][1] - P.tfeat_off[0][0]) == 70 and int(P.tfeat_off[1][1] - P.tfeat_off[1][0]) == 33 and int(P.tfeat_off[2][1] - P.tfeat_off[2][0]) == 7
        if name == "border":
            # plane 0's features spread over a frame around the image at every level (their reference intensities stay: any numbers do): taps leave the
            # image on each of its four borders, others stay inside, and the group stays active (its box is where it was)
            for l in range(P.n_levels):
                h, w = P.img[l][0].shape[-2:]
                f0, f1 = int(P.tfeat_off[l][0]), int(P.tfeat_off[l][1]); n = f1 - f0
                q = np.arange(n)
                side = q % 4
                along = (q // 4 + 0.37)/max(1, (n + 3)//4)
                uv = np.empty((n, 2))
                uv[:, 0] = np.where(side == 0, -1.5, np.where(side == 1, w - 0.5, along*w))
                uv[:, 1] = np.where(side == 2, -1.5, np.where(side == 3, h - 0.5, along*h))
                uv[side < 2, 1] = np.clip(uv[side < 2, 1], 8, h - 9); uv[side >= 2, 0] = np.clip(uv[side >= 2, 0], 8, w - 9)
                P.tfeat_uv[l][f0:f1] = uv
            sides = _tap_sides(P, 0)
            print("border: level-0 taps of plane 0 off the left / right / top / bottom, inside:", sides)
            assert np.all(sides > 0), sides
        elif name == "sigma0":                                  # (the box of plane 1 projects outside every image: sigma = 0, an inactive group)
            P.text_box_ray[1] += 50.0
        else:
            assert name == "base"
    _problems[name] = P
    return P


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(gpu, P, o, variant):
    gpu.debug_set(trial_launches=variant)
    gpu.upload(P, o)
    rs = gpu.reduced_system(o.initial_radius)
    G = P.copy(); rep = gpu.solve(); gpu.download(G)
    return rs, rep, G


@pytest.mark.parametrize("filter_good", [1, 0])
@pytest.mark.parametrize("case", ["base", "border", "sigma0", "frozen", "hosted", "golden"])
def test_carried_projection_equals_second_projection(gpu, case, filter_good):
    """Production (trial_launches = 0) against the partner (4), interleaved (0, 4, 0): S, g and cost of the first linearisation and everything a solve leaves,
    bit for bit.
    base:   5 keyframes, 200 points, 4 planes of 70 / 33 / 7 features at the three levels -- level 0 runs the chunk loop twice (the second chunk's parked
            projections overwrite the area the first chunk's transposes used), and a chunk's last wave holds lanes without a feature.
    border: one plane's taps off each of the four image borders and inside (asserted on the host with synth.text_tap_uv).
    sigma0: one plane's box outside every image -- sigma = 0, the group is inactive and parks nothing.
    frozen / hosted: all text hosts outside / inside the window.        golden: the problem of tests/golden/tiny_local.npz.
    filter_good = 0: the good flags are not consulted."""
    P = _problem(case)
    o = abi.options_local(); o.filter_good = filter_good
    try:
        runs = [_run(gpu, P, o, v) for v in (0, 4, 0)]
    finally:
        gpu.debug_set()
    (rs0, rep0, G0), (rs4, rep4, G4), (rs0b, rep0b, G0b) = runs
    assert sum(rep4["iters"]) > 0 and all(r[1]["poll_timeouts"] == 0 for r in runs)
    assert np.any(rs4["S"] != 0) and rs4["cost"] > 0
    print(case, filter_good, "iters", rep4["iters"], "cost1", rep4["cost1"])
    for what, (rs, rep, G) in (("production", runs[0]), ("production again", runs[2])):
        for k in ("S", "g", "free", "dp"):
            assert np.array_equal(_bits(rs[k]), _bits(rs4[k])), (what, "reduced system", k, np.abs(rs[k] - rs4[k]).max())
        assert rs["cost"] == rs4["cost"], (what, rs["cost"], rs4["cost"])
        for f in REPORT_FIELDS:
            assert rep[f] == rep4[f], (what, f, rep[f], rep4[f])
        for f in PARAMS:
            assert np.array_equal(_bits(getattr(G, f)), _bits(getattr(G4, f))), (what, f)
