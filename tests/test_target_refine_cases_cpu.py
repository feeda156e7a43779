"""The cases of the target step (tests/target_refine_cases.py) on the reference alone (tests/target_refine_ref.py): they promise what they say --
statuses, counts, gauge ranks --, the compared values sit well away from the pivot thresholds, the reference's Jacobians mean what the definition
says (central differences of the generator's projection), and its two routes agree closely enough for the bound to bind."""
import numpy as np
import pytest

import select_ref as sref
import target_refine_cases as tc
import target_refine_ref as ref


@pytest.mark.parametrize("name", tc.NAMES)
def test_two_routes_agree_and_the_bound_binds(name):
    b, s = tc.bounds(name)
    r = tc.reference(name)
    print(name, {k: "%.2e" % v for k, v in s.items() if k != "per_quantity"}, "cost %.3e decrease %.3e |d| %.2e" % (r["cost"], r["predicted_decrease"], np.abs(r["d"]).max()))
    assert b["refined"] <= 1e-7, ("a case is too badly conditioned for a bound on metres to mean anything: replace it", name, s)
    if name in tc.COMPARED:                                            # the step itself is far above the bound, so a wrong step cannot hide inside it
        assert np.abs(r["d"]).max() >= 1e3 * b["refined"], (name, np.abs(r["d"]).max(), b["refined"])
        assert b["cost"] <= 1e-6 * r["cost"] and b["predicted_decrease"] <= 1e-3 * r["predicted_decrease"], (name, b, r["cost"], r["predicted_decrease"])
    assert r["predicted_decrease"] >= 0.0


@pytest.mark.parametrize("name", ["mono_fov", "mono_poly2", "mono_poly3", "mono_kb4", "mono_linear", "mono_rational6", "stereo_fov"])
def test_jacobians_against_central_differences(name):
    """the analytic rows against central differences at two steps: 4 x the steps' own disagreement is allowed, per block, relative to the block's largest entry"""
    case = tc.cases()[name]
    views = ref.views_of(case)
    worst = 0.0
    for f in (0, 1):
        for c, ids, z in views[f]:
            a = ref.rows_analytic(case, f, c, ids, z)
            n1, n2 = ref.rows_numeric(case, f, c, ids, z, tc.H1), ref.rows_numeric(case, f, c, ids, z, tc.H2)
            for k in range(3):
                if a[k].size == 0:
                    continue
                scale = np.abs(a[k]).max(axis=0 if k < 2 else (0, 1), keepdims=True)
                tol = 4.0 * np.abs((n1[k] - n2[k]) / scale).max() + 1e-9
                err = np.abs((a[k] - n2[k]) / scale).max()
                worst = max(worst, err / tol)
                assert err <= tol, (name, f, c, k, err, tol)
            assert np.abs(a[3] - n2[3]).max() <= 1e-9
    print(name, "worst of error / tolerance %.3f" % worst)


def test_statuses_are_what_the_cases_say():
    r = tc.reference("p117_views")
    assert r["frame_status"].tolist() == [1, 0, 0, 0, 0] and r["corners"].tolist() == [3, 4, 63, 64, 65]
    assert (r["point_status"] == 1).any() and (r["point_corners"][r["point_status"] == 1] == 0).all()
    r, sp = tc.reference("mixed"), tc.cases()["mixed"]["special"]
    assert r["point_corners"][sp["one_view"]] == 1 and r["point_status"][sp["one_view"]] == 0
    assert r["point_status"][sp["never"]] == 1 and r["point_status"][sp["behind"]] == 1
    assert r["frame_status"][sp["behind_frame"]] == 2 and r["behind"][sp["behind_frame"]] == 1 and r["behind"].sum() == 1
    assert np.array_equal(r["refined"][[sp["never"], sp["behind"]]], tc.cases()["mixed"]["points"][[sp["never"], sp["behind"]]])
    assert tc.reference("collinear")["gauge_rank"] == 6
    for n in tc.NAMES:
        r = tc.reference(n)
        assert r["gauge_rank"] == tc.EXPECT_RANK.get(n, 7) and r["result_status"] == ref.OK, n
    st = tc.cases()["stereo_fov"]
    v = ref.views_of(st)
    assert len(v[0]) == 2 and len(set(v[0][0][1]) & set(v[0][1][1])) >= 20 and len(v[1]) == 1
    assert sref.dim(tc.unsupported_case()["cameras"]) == 74
    assert [sref.dim(tc.cases()[n]["cameras"]) for n in ("p4_n1_fixed", "p5_n2_fixed")] == [0, 0]


@pytest.mark.parametrize("name", tc.NAMES)
def test_values_sit_away_from_the_thresholds(name):
    """every usable frame's smallest pivot of J_f^T J_f is >= 1e4 x the status threshold, the 3-corner frame fails on its count; the gauge columns kept
    keep >= 1e-3 of their norm and the one dropped falls below 1e-12; the dense system's smallest eigenvalue is >= 1e4 x the pivot threshold x its
    largest diagonal entry"""
    case = tc.cases()[name]
    frames, status, corners, behind, _ = ref.frame_rows(case)
    for fr, st, n in zip(frames, status, corners):
        if st == 1:
            assert n < 4, (name, "a frame is refused by its pivots: the case should say so")
            continue
        H = fr["Jf"].T @ fr["Jf"]
        L = np.linalg.cholesky(H)
        assert (np.diag(L) ** 2).min() >= 1e4 * ref.PIVOT_TOL * np.diag(H).max(), name
    r = tc.reference(name)
    obs = np.where(r["point_status"] == 0)[0]
    nominal = case["nominal"]
    u = nominal[obs] - nominal[obs].mean(axis=0)
    cols = [np.tile(e, len(u)) for e in np.eye(3)] + [np.cross(e, u).reshape(-1) for e in np.eye(3)] + [u.reshape(-1)]
    Q = []
    for q in cols:
        q = q.copy(); before = np.linalg.norm(q)
        for k in Q:
            q -= (k @ q) * k
        ratio = np.linalg.norm(q) / before if before > 0 else 0.0
        assert ratio >= 1e-3 or ratio <= 1e-12, (name, ratio)
        if ratio >= 1e-3:
            Q.append(q / np.linalg.norm(q))
    assert r["pivot_margin"] >= 1e4 * ref.PIVOT_TOL, (name, r["pivot_margin"])


def test_similarity_in_points_changes_nothing():
    """the reference itself.  A similarity delta added to `points` moves the point of linearisation: the data term's null space follows it, so
    `refined` moves by about |delta| |d| / (the board's size) -- the step d turns with the board -- and by the projection's second order, about
    (6.5e3 px / m^2) |delta|^2 / (1e3 px / m).  The statement is therefore checked where d = 0, on the exact case, with |delta| <= 2e-8 m: the second
    order is then 3e-15 m, below the bound, while delta itself is >= 1e5 bounds: a step that did not project it out would miss by that much."""
    case = tc.moved_by_small_similarity("exact")
    base, moved = tc.reference("exact"), ref.step(case)
    b = tc.bounds("exact")[0]["refined"]
    assert np.abs(case["points"] - tc.cases()["exact"]["points"]).max() >= 1e5 * b
    print("moved by %.3e m, bound %.3e m" % (np.abs(moved["refined"] - base["refined"]).max(), b))
    assert np.abs(moved["refined"] - base["refined"]).max() <= b
