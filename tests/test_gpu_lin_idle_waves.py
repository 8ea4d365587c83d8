"""A wave of a text workgroup of k_linearize that holds no feature of a 64-feature chunk goes round the chunk's work (tsba_kernels_lin.h, lin_body): no clamped
feature loads, no pixel fetches, no tap loop, no transposes -- it meets the chunk's barriers and hands +0.0 to the cross-wave sum.  The partner
(tsba_debug_options.trial_launches = 5, lin_body<.., LIN_ALLW>) keeps every wave evaluating: a wave without a feature on the group's clamped last feature under
weight 0.  The live lanes' expressions and the order of the sums are the same, and the idle wave's share was a sum of x * 0.0 terms, so the two agree in VALUE
everywhere (np.array_equal: -0 == +0 -- the old idle wave could hand on -0, which shows only where wave 0's own sum is an exact zero, the all-bad group below):
the reduced system of the first linearisation (S, g, cost) and everything a whole solve leaves (parameters, flags, report, the LM trace of each pass).
A level whose largest text group fits one wave (at most 32 features) is launched with one-wave workgroups (64 threads: a scene workgroup takes one pair, the
cross-wave sum has one term) where a wave takes a whole (target, host) pair; the partner keeps 128 threads everywhere, so the same comparison covers that
path, and tsba_debug_solver_info's per-level read-out (Optimizer.linearize_threads) says which width each level's launch takes."""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

# features per plane at levels 0 / 1 / 2.  A text workgroup has two waves of 32 feature places and walks a group in chunks of 64.
SHAPES = {
    "idle_all": (12, 8, 6),           # wave 1 idle on every level
    "full_wave0": (32, 24, 12),       # exactly a full wave 0
    "one_in_wave1": (33, 32, 31),     # one feature in wave 1, then none
    "c4": (64, 24, 12),               # the benchmark window's shape: both waves full at level 0
    "chunk2_of_6": (70, 33, 7),       # second chunk of 6: wave 1 idle in chunk 2 only
    "chunk2_of_32": (96, 40, 12),     # second chunk of exactly 32
}
# (problem, filter_good, lds_poison)
CASES = {name: (name, 1, 0) for name in SHAPES}
CASES.update({
    "sigma0": ("sigma0", 1, 0),               # one plane's box outside every image: sigma = 0, an inactive group -- both its waves go round the work
    "all_bad": ("all_bad", 1, 0),             # every feature of one (keyframe, plane) group flagged bad: wave 0's own sums are exact zeros (the zero-sign case)
    "no_filter": ("idle_all", 0, 0),          # the good flags are not consulted
    "frozen": ("frozen", 1, 0),               # every text host outside the window (pair_from_Twr)
    "hosted": ("hosted", 1, 0),               # every text host a keyframe of the window (pair_from_poses)
    "lds_poison": ("idle_all", 1, 1),         # LDS full of NaNs before every launch of the solves: a wave that reads what it has not written changes the result
})
REPORT_FIELDS = ("iters", "accepted", "termination", "cost0", "cost1", "n_sblock", "n_tblock", "n_bad_scene", "n_bad_tfeat", "n_bad_text")
PARAMS = ("pose", "rho", "theta", "sgood", "tobs_good", "tfgood")
_problems = {}


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


def _problem(name):
    if name in _problems:
        return _problems[name]
    if name in SHAPES:
        feats = SHAPES[name]
        P = synth.tiny(feats=feats)                             # 5 keyframes, 60 points, 4 planes, three levels
    elif name == "frozen":
        feats = SHAPES["chunk2_of_6"]
        P = synth.tiny(feats=feats, frozen_frac=1.0)
        assert np.all(P.text_host < 0)
    elif name == "hosted":
        feats = SHAPES["chunk2_of_6"]
        P = synth.tiny(feats=feats, frozen_frac=0.0)
        assert np.all(P.text_host >= 0)
    elif name == "sigma0":
        feats = SHAPES["idle_all"]
        P = synth.tiny(feats=feats)
        P.text_box_ray[1] += 50.0
    else:
        assert name == "all_bad"
        feats = SHAPES["idle_all"]
        P = synth.tiny(feats=feats)
        # (an observation from another keyframe than the plane's host: the host's own observation forms no group)
        t = int(np.nonzero((P.tobs_good == 1) & (P.tobs_kf != P.text_host[P.tobs_text]))[0][0])
        P.tfgood[int(P.tobs_fgood_off[t]):int(P.tobs_fgood_off[t + 1])] = 0
    assert P.n_levels == 3 and P.n_text == 4
    for l in range(3):
        assert np.all(np.diff(P.tfeat_off[l]) == feats[l]), (name, l, np.diff(P.tfeat_off[l]))
    _problems[name] = P
    return P


def _run(gpu, P, o, variant, poison, no_small_pairs):
    gpu.debug_set(trial_launches=variant, lds_poison=poison, no_small_pairs=no_small_pairs)
    gpu.upload(P, o)
    rs = gpu.reduced_system(o.initial_radius)
    G = P.copy(); rep = gpu.solve(); gpu.download(G)
    trace = [gpu.lm_trace(ps) for ps in range(o.n_passes)]
    return rs, rep, G, trace, gpu.linearize_threads(), gpu.solver_info()["small_pairs"]


@pytest.mark.parametrize("pairs", ["four_pairs_per_wave", "wave_per_pair"])
@pytest.mark.parametrize("case", list(CASES))
def test_idle_wave_skip_equals_every_wave_evaluating(gpu, case, pairs):
    """Production (trial_launches = 0) against the partner (5), interleaved (0, 5, 0) on one context: S, g and cost of the first linearisation, the parameters
    and flags a solve leaves, its report and the LM trace of every pass, value for value; no poll of a solve ran into its bound.
    four_pairs_per_wave: the path these small problems take by themselves (a dozen scene blocks per pair: four pairs share a wave, 128-thread workgroups on every
    level).  wave_per_pair (no_small_pairs = 1): the benchmark window's path -- production takes 64-thread workgroups on every level whose planes have at most
    32 features and 128 elsewhere, the partner 128 everywhere (asserted through the read-out)."""
    pname, filter_good, poison = CASES[case]
    P = _problem(pname)
    o = abi.options_local(); o.filter_good = filter_good
    try:
        runs = [_run(gpu, P, o, v, poison, pairs == "wave_per_pair") for v in (0, 5, 0)]
    finally:
        gpu.debug_set()
    feats = [int(P.tfeat_off[l][1] - P.tfeat_off[l][0]) for l in range(3)]
    print(case, pairs, "features by level", feats, "threads by level: production", runs[0][4], "partner", runs[1][4], "four pairs per wave", runs[0][5])
    assert [r[5] for r in runs] == [int(pairs == "four_pairs_per_wave")]*3
    assert runs[1][4] == [128, 128, 128]
    assert runs[0][4] == runs[2][4] == ([128, 128, 128] if pairs == "four_pairs_per_wave" else [64 if n <= 32 else 128 for n in feats])
    rs5, rep5, G5, tr5 = runs[1][:4]
    assert all(r[1]["poll_timeouts"] == 0 for r in runs), [r[1]["poll_timeouts"] for r in runs]
    assert sum(rep5["iters"]) > 0 and np.any(rs5["S"] != 0) and rs5["cost"] > 0
    print(case, "iters", rep5["iters"], "accepted", rep5["accepted"], "cost0", rep5["cost0"], "cost1", rep5["cost1"])
    if case == "all_bad":                                       # (the flagged group is one that counted: without the flags the first linearisation costs more)
        gpu.upload(_problem("idle_all"), o)
        assert gpu.reduced_system(o.initial_radius)["cost"] > rs5["cost"]
    for what, (rs, rep, G, tr) in (("production", runs[0][:4]), ("production again", runs[2][:4])):
        for k in ("S", "g", "free", "dp"):
            assert np.array_equal(rs[k], rs5[k]), (what, "reduced system", k, np.abs(rs[k] - rs5[k]).max())
        assert rs["cost"] == rs5["cost"], (what, rs["cost"], rs5["cost"])
        for f in REPORT_FIELDS:
            assert rep[f] == rep5[f], (what, f, rep[f], rep5[f])
        for f in PARAMS:
            assert np.array_equal(getattr(G, f), getattr(G5, f)), (what, f)
        for ps in range(o.n_passes):                            # (a trial with an invalid step records NaN as its cost: in both or in neither)
            assert tr[ps].shape == tr5[ps].shape and np.array_equal(tr[ps], tr5[ps], equal_nan=True), (what, "LM trace of pass", ps, tr[ps], tr5[ps])
