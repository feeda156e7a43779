"""The odd-even elimination order of a chain group (vicalib_amd/csrc/vc_chain_order.hpp), built for the host by tests/host_harness:
(a) the schedule's invariants for every group shape, (b) a bordered block-tridiagonal system eliminated and back-substituted in the
schedule's order against a dense solve."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def H():
    src = os.path.join(HERE, "host_harness", "chain_order_harness.cpp")
    so = os.path.join(HERE, "host_harness", "libvc_chain_order_harness.so")
    deps = [src] + [os.path.join(ROOT, "vicalib_amd", "csrc", f) for f in ("vc_chain_order.hpp", "vc_chain_plan.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _consts(H):
    out = (C.c_int * 5)()
    H.vc_oe_consts(out)
    return dict(left_sep=out[0], right_sep=out[1], nobody=out[2], waves=out[3], max_q=out[4])


def _frame(H, q, hl, hr, i):
    out = (C.c_int * 4)()
    H.vc_oe_frame(q, int(hl), int(hr), i, out)
    return dict(step=out[0], left=out[1], right=out[2], wave=out[3])


SHAPES = [(q, hl, hr) for q in range(1, 8) for hl in (False, True) for hr in (False, True)]


@pytest.mark.parametrize("q,hl,hr", SHAPES)
def test_schedule_invariants(H, q, hl, hr):
    k = _consts(H)
    assert k["max_q"] == 7 and k["waves"] == 4
    fr = {i: _frame(H, q, hl, hr, i) for i in range(1, q + 1)}
    steps = H.vc_oe_steps(q)
    assert steps == math.ceil(math.log2(q + 1))
    # every interior index is eliminated exactly once, in a round 1 .. steps, and every round has somebody
    assert all(1 <= f["step"] <= steps for f in fr.values())
    assert {f["step"] for f in fr.values()} == set(range(1, steps + 1))
    # the rule itself
    for i, f in fr.items():
        h = 1 << (f["step"] - 1)
        assert i % h == 0 and (i // h) % 2 == 1
        assert f["left"] == (i - h if i - h >= 1 else (k["left_sep"] if hl else k["nobody"]))
        assert f["right"] == (i + h if i + h <= q else (k["right_sep"] if hr else k["nobody"]))
    # a frame's neighbours are still there at its round; no two frames of one round are neighbours of each other
    for i, f in fr.items():
        for nb in (f["left"], f["right"]):
            if nb >= 1:
                assert fr[nb]["step"] > f["step"]
    # no wavefront is given two frames in one round, none holds more than two frames, and all fit the workgroup
    for st in range(1, steps + 1):
        waves = [f["wave"] for f in fr.values() if f["step"] == st]
        assert len(waves) == len(set(waves))
    for w in range(k["waves"]):
        assert sum(1 for f in fr.values() if f["wave"] == w) <= 2
    assert all(0 <= f["wave"] < k["waves"] for f in fr.values())
    # the last round is one frame, the one oe_last names, and it sees the separators (or nobody) on both sides
    last = [i for i, f in fr.items() if f["step"] == steps]
    assert last == [H.vc_oe_last(q)]
    assert fr[last[0]]["left"] < 1 and fr[last[0]]["right"] < 1


def _system(rng, t, hl, hr, nb):
    """SPD block-tridiagonal chain of P 9 x 9 blocks with a dense border of nb columns; well conditioned by construction: unit-scale
    diagonal blocks 4 I + small symmetric noise, couplings of entries below 0.15 -- Gershgorin keeps the spectrum inside (4 - 3.6, 4 + 3.6)."""
    P = t + int(hl) + int(hr)
    n = P * 9 + nb
    A = np.zeros((n, n))
    for p in range(P):
        S = rng.uniform(-0.05, 0.05, (9, 9))
        A[p * 9:(p + 1) * 9, p * 9:(p + 1) * 9] = 4.0 * np.eye(9) + 0.5 * (S + S.T)
        if p + 1 < P:
            Bk = rng.uniform(-0.12, 0.12, (9, 9))
            A[p * 9:(p + 1) * 9, (p + 1) * 9:(p + 2) * 9] = Bk
            A[(p + 1) * 9:(p + 2) * 9, p * 9:(p + 1) * 9] = Bk.T
        W = rng.uniform(-0.12, 0.12, (9, nb))
        A[p * 9:(p + 1) * 9, P * 9:] = W
        A[P * 9:, p * 9:(p + 1) * 9] = W.T
    S = rng.uniform(-0.05, 0.05, (nb, nb))
    A[P * 9:, P * 9:] = 4.0 * np.eye(nb) + 0.5 * (S + S.T) + 0.12 * 0.12 * 9 * P * np.eye(nb)
    return A, rng.uniform(-1.0, 1.0, n)


@pytest.mark.parametrize("t,hl,hr", [(t, hl, hr) for t in range(1, 8) for hl, hr in itertools.product((False, True), repeat=2)])
def test_elimination_in_schedule_order_matches_dense_solve(H, t, hl, hr):
    rng = np.random.default_rng(1000 + 4 * t + 2 * int(hl) + int(hr))
    nb = 5
    A, g = _system(rng, t, hl, hr, nb)
    cond = np.linalg.cond(A)
    print("t = %d, separators %d / %d: n = %d, condition number %.1f" % (t, hl, hr, len(g), cond))
    assert cond < 1e4
    ref = np.linalg.solve(A, g)
    x = np.zeros_like(g)
    rc = H.vc_oe_solve(t, int(hl), int(hr), nb, A.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    assert rc == 0
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print("relative error %.3e" % err)
    assert err <= 1e-11


def _plan(H, N, D, sharded=False, odd_even=True):
    out = (C.c_int * 34)()
    H.vc_oe_plan(N, D, 1, 1, int(sharded), int(odd_even), out)
    nl = out[0]
    return dict(n_levels=nl, oe_top=out[1], oe=[out[2 + l] for l in range(nl)], two=[out[18 + l] for l in range(nl)])


@pytest.mark.parametrize("N", [7, 57, 130, 648, 2000, 4097])
def test_plan_marks_the_levels_above_the_bottom_one(H, N):
    p = _plan(H, N, 29)
    assert p["oe_top"] == 1
    assert p["oe"] == [1 if l >= 1 else 0 for l in range(p["n_levels"])]
    assert p["two"] == [1] * p["n_levels"]                                      # what the levels run with the switch off keeps its value
    for other in (_plan(H, N, 29, odd_even=False), _plan(H, N, 29, sharded=True), _plan(H, N, 37), _plan(H, N, 115)):
        # the switch off, a sharded pass, borders of more than one column per lane (D + 28 > 64): today's kernels
        assert other["oe_top"] == 0 and not any(other["oe"])
        assert other["n_levels"] == p["n_levels"]
