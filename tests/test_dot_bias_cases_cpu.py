"""What tests/dot_bias_cases.py promises, asserted on the numpy reference (tests/dot_bias_ref.py) alone: no library, no GPU."""
import numpy as np

import dot_bias_cases as dc
import dot_bias_ref as ref


def test_the_bound_and_what_bound_asserts():
    b, spreads = dc.bound()          # (asserts the statuses, the exact ellipse centres on `linear`, the fronto-parallel zero, the radii in pixels)
    assert set(spreads) == set(dc.GROUPS) and 0.0 < b <= 1e-6
    print("bound %.3e px; spreads %s" % (b, {k: "%.2e" % v for k, v in spreads.items()}))


def test_the_cases_cover_what_they_claim():
    g = dc.group("models")
    assert [len(v["radius"]) for v in g["views"]] == dc.SIZES and sum(dc.SIZES) == 257 and dc.SIZES.count(0) == 3
    assert [v["model"] for v in g["views"]] == dc.MODELS * 2
    for n in dc.PREFIXES:
        arrays, rows = dc.prefix(n)
        assert len(arrays[5]) == n == len(rows) and arrays[3][-1] == n and len(arrays[0]) == 12
    assert sorted(v["model"] for v in dc.group("axis")["views"]) == sorted(dc.MODELS)
    for v in dc.group("axis")["views"]:          # the centre sits on the optical axis exactly
        pc = dc.synth.quat_to_matrix(v["T_cw"][:4]) @ v["pw"][0] + v["T_cw"][4:]
        assert pc[0] == 0.0 and pc[1] == 0.0 and pc[2] > 0.0
    assert set(np.unique(dc.group("models")["views"][3]["radius"])) == {dc.R_LARGE, dc.R_SMALL}
    status = dc.reference("status")["status"].tolist()
    assert status == [ref.NO_CENTRE, ref.NO_CENTRE, ref.NO_RIM, ref.OK, ref.NO_CENTRE, ref.LEFT_DOT, ref.OK]
    assert np.isnan(dc.group("status")["views"][2]["T_cw"]).sum() == 1
    tilt = dc.group("sizes")["views"][3]["T_cw"]
    assert abs(2.0 * np.degrees(np.arctan2(np.linalg.norm(tilt[:3]), tilt[3])) - 80.0) < 1e-9


def test_the_bias_has_the_size_the_design_quotes():
    """pinhole f = 420 px, the 9.4 mm dot (about 10 px) at 0.42 m and a tilt of 0.5 rad: about a tenth of a pixel; the board over the views of `models`:
    some hundredths rms"""
    st, bias, s = ref.one(ref.LINEAR, np.array(dc.PARAMS["linear"] + [0.0] * 6), dc.pose([0.5, 0.0, 0.0], [0.0, 0.0, 0.42]), np.array([0.06, 0.045, 0.0]), dc.R_LARGE)
    assert st == ref.OK and 0.05 < np.linalg.norm(bias) < 0.2 and 7.0 < s < 11.0
    r = dc.reference("models")
    rms = np.sqrt(np.mean(np.sum(r["bias"] ** 2, axis=1)))
    assert 0.01 < rms < 0.2, rms


def test_sixty_four_samples_are_enough():
    """the 64-sample centre against a 4096-sample one, on the pinhole and on the kb4 lens"""
    worst = 0.0
    for v in dc.group("models")["views"]:
        if v["model"] not in ("linear", "kb4") or not len(v["radius"]):
            continue
        K = np.zeros(10); K[:len(v["params"])] = v["params"]
        for C, rr in list(zip(v["pw"], v["radius"]))[:6]:
            a = ref.one(dc.synth.MODEL_IDS[v["model"]], K, v["T_cw"], C, rr, n=64)
            b = ref.one(dc.synth.MODEL_IDS[v["model"]], K, v["T_cw"], C, rr, n=4096)
            assert a[0] == b[0] == ref.OK
            worst = max(worst, float(np.abs(a[1] - b[1]).max()))
    print("64 against 4096 samples: %.3e px" % worst)
    assert worst < 1e-9
