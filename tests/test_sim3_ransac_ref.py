"""The numpy restatement of Sim3Solver (tests/sim3_ransac_ref.py) against what it must be by construction: exact data, the selection rule, the
hypothesis-count rule, a degenerate triple, the draw scheme, and the table a prototype of the test world's recipe gave."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ransac_ref as S


def _exact(seed, n=40):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    R = S.quat_to_R(q); t = rng.uniform(-0.5, 0.5, 3); s = rng.uniform(0.7, 1.4)
    P2 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.5, 7.0, n)], 1)
    P1 = s*(P2 @ R.T) + t
    return q, R, t, s, P1, P2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exact_data_every_hypothesis_is_the_transform(seed):
    q, R, t, s, P1, P2 = _exact(seed)
    K = np.array([384.396254546, 382.825746531, 315.635886103, 249.182929809])
    g = np.random.default_rng(seed)
    tri = S.draw_triples(len(P1), 5, lambda lo, hi: lo + int(g.random()*(hi - lo + 1)))
    assert len(set(tri.reshape(-1).tolist())) == 15                    # the list of available indices is not refilled
    res = S.ransac(P1, P2, S.pred_of(P1, K), S.pred_of(P2, K), tri, K, K)
    for h in res["hyps"]:
        np.testing.assert_allclose(h["R"], R, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h["q"], q, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h["t"], t, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h["s"], s, rtol=1e-12)
        np.testing.assert_allclose(h["T21"][:, :3] @ h["T12"][:, :3], np.eye(3), atol=1e-12)
    assert res["counts"] == [len(P1)]*5 and res["sel"] == 4 and res["ok"] and res["mask"].all()


def test_selection_rule():
    assert S.select([43, 0, 43, 30, 43]) == (4, 43, True)              # `>=`: the later of equal counts wins
    assert S.select([0, 0, 0]) == (2, 0, False)                        # a hypothesis without inliers is still "selected"
    assert S.select([21])[2] is True and S.select([20])[2] is False    # ok = best > min_inliers, strict
    assert S.select([]) == (-1, 0, False)


def test_hypothesis_count_rule():
    assert [S.n_hypotheses(n) for n in (0, 19, 20, 21, 22)] == [0, 0, 1, 3, 4]
    assert all(S.n_hypotheses(n) == 5 for n in list(range(24, 400)) + [1500, 100000])


def test_degenerate_triple_has_no_inliers():
    q, R, t, s, P1, P2 = _exact(3)
    K = np.array([384.4, 382.8, 315.6, 249.2])
    P1 = P1.copy(); P2 = P2.copy(); P1[1] = P1[2] = P1[0]; P2[1] = P2[2] = P2[0]
    res = S.ransac(P1, P2, S.pred_of(P1, K), S.pred_of(P2, K), [[0, 1, 2]], K, K)
    assert res["counts"] == [0] and res["sel"] == 0 and not res["ok"] and not res["mask"].any()
    # exactly equal relative coordinates (all zero): s = 0 / 0, every comparison with NaN is false
    Z = np.zeros((3, 3)); P1[:3] = Z + [0.0, 0.0, 4.0]; P2[:3] = Z + [0.0, 0.0, 4.0]
    res = S.ransac(P1, P2, S.pred_of(P1, K), S.pred_of(P2, K), [[0, 1, 2]], K, K)
    assert np.isnan(res["hyps"][0]["s"]) and res["counts"] == [0] and not res["ok"]


def test_lcg_draws_stay_in_range_and_are_distinct():
    g = S.Lcg32(7)
    tri = S.draw_triples(21, 3, g.random_int)
    assert tri.shape == (3, 3) and len(set(tri.reshape(-1).tolist())) == 9 and tri.min() >= 0 and tri.max() < 21
    assert np.array_equal(tri, S.draw_triples(21, 3, S.Lcg32(7).random_int))


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "seed%d" % c[0])
def test_world_gives_the_prototypes_table(case):
    w = S.world(*case); res = S.run_world(w)
    counts, sel, ok, _ = S.EXPECT[case[0]]
    assert res["counts"][:8] == counts and res["sel"] == sel and res["ok"] == ok
    assert len(res["counts"]) == case[3]
    c = S.conditions(w, res)
    assert c["err_margin"] >= 1e-5 and c["gap"] >= 1e-3
