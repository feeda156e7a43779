"""Worker of tests/test_lm_step_sharded_gpu.py: one held LM step of a frame-sharded pass against the dense reference solve of the whole
problem (tests/lm_step_ref.py).  TEST INFRASTRUCTURE ONLY.

  lm_step_sharded_worker.py <case name> <store directory>

The P ranks of a case run as threads of this one process, one calibrator each (several calibrators per process, as full_size_worker.py
hosts them), and every rank all-reduces through a gloo group of its own set up through a file store.  Rank r loads frames
frame_shard(N, r, P) of one generated problem and the whole IMU stream.  The ranks run every device call first -- one linearize(), then
step_hold() at each radius, all ranks together -- and the main thread compares what they read out with the oracle afterwards.  A failing
rank prints WORKER-FAILURE and ends the process: its peers would otherwise wait in their all-reduces until the group's time-out."""
import datetime
import os
import sys
import threading
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import lm_step_ref as ref        # noqa: E402
from test_lm_step_gpu import _block_check      # noqa: E402
from vicalib_amd import synth    # noqa: E402
from vicalib_amd.parallel import frame_shard      # noqa: E402

RADII = (1e0, 1e4, 1e8)
EPS = np.finfo(np.float64).eps
ALL_FLAGS = (True, True, False, True)
SENTINEL = -7.77e77
PAD = 64


def _v(models, n, P, D, drop=(), seed=37, env=None):
    # vision only from the initial estimate, as test_lm_step_gpu's vision cases: at the ground truth the gradient is a sum of noise-level
    # terms that cancel, so its own rounding (g_s to ~4e-12 relative between the device's and the oracle's summation order, measured on
    # these cases) enters the step as kappa times that -- an error of the linearisation, outside what the solve's bound accounts for
    return dict(kind="vision", models=models, n=n, P=P, D=D, drop=tuple(drop), seed=seed, env=env or {}, flags=None, init=True, paths=None)


def _i(models, n, P, D, flags=ALL_FLAGS, seed=5, paths=None, env=None, init=False, drop=()):
    return dict(kind="vi", models=models, n=n, P=P, D=D, drop=tuple(drop), seed=seed, env=env or {}, flags=flags, init=init, paths=paths)


CFG5 = ("fov", "kb4") * 4
CASES = {
    # vision only: the sharded vision pass, no separators (D = D0)
    "vision_2": _v(("fov", "poly3"), 40, 2, 18),
    "vision_3_uneven_empty_first": _v(("fov", "poly3"), 40, 3, 18, drop=(13,)),          # shards 13 / 13 / 14; rank 1's first frame unobserved
    # the split kernels of a sharded pass on one rank: no separators
    "force_shard_vision_1": _v(("fov", "poly3"), 40, 1, 18, env=dict(VICALIB_AMD_FORCE_SHARD_PATH="1")),
    "force_shard_vi_1": _i(("kb4",), 40, 1, 29, env=dict(VICALIB_AMD_FORCE_SHARD_PATH="1")),
    # separators: D = D0 + 9 (P - 1)
    "vi_mono_sep_in_one_wavefront": _i(("fov",), 40, 2, 23, flags=(False, True, False, True)),      # D0 = 14: the one-wavefront solve
    "vi_kb4_2": _i(("kb4",), 40, 2, 38),
    "vi_kb4_3": _i(("kb4",), 40, 3, 47),                    # the middle rank holds a separator and a ghost
    "vi_kb4_8x2": _i(("kb4",), 16, 8, 92),                  # shards of 2 frames
    "vi_kb4_8x2_odd": _i(("kb4",), 17, 8, 92),              # the last shard has an interior frame
    "vi_kb4_2x57": _i(("kb4",), 114, 2, 38),                # chain group boundaries on each side
    "vi_kb4_2x64": _i(("kb4",), 128, 2, 38),
    "vi_kb4_2x65": _i(("kb4",), 130, 2, 38),
    "vi_kb4_3_back_levels": _i(("kb4",), 132, 3, 47, paths=dict(back_path=0), env=dict(VICALIB_AMD_BACK_PATH="0")),
    "vi_kb4_2x520": _i(("kb4",), 1040, 2, 38, paths=dict(back_path=1, tail_deferred=1)),
    "vi_kb4_3_empty_separator": _i(("kb4",), 40, 3, 47, drop=(13,)),    # rank 1's separator: IMU blocks only
    "vi_rotation_only": _i(("fov", "kb4"), 40, 2, 44, flags=(True, True, True, True), init=True),
    "vi_biases_inactive": _i(("fov", "kb4"), 40, 2, 37, flags=(False, True, False, True)),
    # the register-tiled reduced solve at the widths only sharded passes reach
    "vi_cfg5_2": _i(CFG5, 66, 2, 124),
    "vi_cfg5_4": _i(CFG5, 66, 4, 142),
    "vi_cfg5_6": _i(CFG5, 66, 6, 160),                      # exactly 10 row tiles
    "vi_cfg5_8": _i(CFG5, 66, 8, 178),
    "vi_r6x7_poly3_5": _i(("rational6",) * 7 + ("poly3",), 66, 5, 176),      # exactly 11 row tiles
    "vi_r6x7_kb4_5": _i(("rational6",) * 7 + ("kb4",), 66, 5, 177),          # the 12th row tile has one row
    "vi_r6x8_5": _i(("rational6",) * 8, 66, 5, 179),                          # the limit
}
# one past the limit: cfg5's rig with one fov camera replaced by poly3 is D0 = 117, over 8 ranks D = 180
LIMIT_MODELS = ("poly3", "kb4") + ("fov", "kb4") * 3


def problem(case):
    p = synth.generate(synth.Config(models=case["models"], n_frames=case["n"], imu=case["kind"] == "vi", seed=case["seed"]))
    if case["drop"]:
        p.tiles = [t for t in p.tiles if t[0] not in case["drop"]]
    return p


def imu_start(p):
    gt = p.imu_gt
    return np.concatenate([gt["bg"], gt["ba"]]) * 0.7, np.concatenate([gt["sg"], gt["sa"]]) * 1.005, np.array([0.02, 0.01]), 0.0013


def load_slice(cal, p, lo, hi, init):
    """Frames [lo, hi) of p with their observations, and the whole IMU stream (dist_worker.load_slice, with the choice of start)."""
    for c, m in enumerate(p.cam_model):
        cal.AddCamera(m, p.cam_K_init[c] if init else p.cam_K_gt[c], p.cam_T_ck_init[c] if init else p.cam_T_ck_gt[c], p.cfg.width, p.cfg.height)
    T = p.frame_T_wk_init if init else p.frame_T_wk_gt
    for f in range(lo, hi):
        cal.AddFrame(T[f], p.frame_time[f])
    for (f, c, ids, pix) in p.tiles:
        if lo <= f < hi:
            cal.AddObservations(f - lo, c, p.grid_points[ids], pix)
    if p.imu_t is not None:
        cal.AddImuMeasurements(p.imu_gyro, p.imu_accel, p.imu_t)
    return cal


def set_state(cal, case, p):
    if case["kind"] == "vision":
        cal.SetCalibrateImu(False)
        return
    b0, s0, g0, t0 = imu_start(p)
    cal.SetOptimizationFlags(*case["flags"]); cal.SetBiases(b0); cal.SetScaleFactor(s0); cal.SetTimeOffset(t0); cal.SetGravity(g0)


def make_group(store, rank, world):
    import torch.distributed as dist
    return dist.ProcessGroupGloo(dist.PrefixStore("lm_step", dist.FileStore(store, world)), rank, world, datetime.timedelta(seconds=300))


def attach(cal, group, rank, world):
    from vicalib_amd.parallel import FrameShardComm
    comm = FrameShardComm(group=group, device="cuda:0", stream_ptr=cal.stream())
    cal.set_shard(rank, world, comm)
    return comm


def run_ranks(world, body):
    """body(rank) on a thread per rank; a rank that raises ends the process (WORKER-FAILURE)."""
    out = [None] * world

    def run(rank):
        try:
            out[rank] = body(rank)
        except BaseException as e:      # noqa: BLE001
            sys.stdout.flush()
            os.write(1, ("WORKER-FAILURE rank %d: %s\n%s\n" % (rank, type(e).__name__, (str(e) + "\n" + traceback.format_exc())[:6000])).encode())
            os._exit(1)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out


# ---- the held step --------------------------------------------------------------------------------------------------------------

def device_side(case, p, store):
    from vicalib_amd.lib import ViCalibrator
    P = case["P"]

    def body(rank):
        group = make_group(store, rank, P)
        lo, hi = frame_shard(case["n"], rank, P)
        cal = load_slice(ViCalibrator(0), p, lo, hi, case["init"])
        set_state(cal, case, p)
        comm = attach(cal, group, rank, P)
        res = dict(lo=lo, hi=hi)
        res["lin"] = cal.linearize()
        res["D"] = cal.shared_dim()
        res["n_frames"] = cal.NumFrames()
        if case["kind"] == "vi":
            res["paths"] = cal.pass_paths()
            res["n_blocks"] = cal.num_imu_blocks()
            # the first pass linearised with the initial weights and left the ones of this state: linearise again with those
            res["W"] = cal.imu_weights()
            res["lin"] = cal.linearize()
        res["steps"] = [cal.step_hold(radius) for radius in RADII]
        assert comm.calls > 0
        group.barrier().wait()
        cal.close()
        return res

    return run_ranks(P, body)


def check_case(name, store):
    import oracle_lib as ol
    from vicalib_amd.lib import ViCalibrator
    case = CASES[name]
    P, vi = case["P"], case["kind"] == "vi"
    p = problem(case)
    ranks = device_side(case, p, store)
    N = case["n"]
    seps = ref.separator_frames(N, P) if vi and P > 1 else []
    # the oracle on the whole problem, at the same state, with the weights the ranks linearised with
    orc = ol.Oracle().load(p, init=case["init"])
    if vi:
        orc.set_options(calibrate_imu=True); orc.set_flags(*case["flags"]); orc.set_imu_state(*imu_start(p))
        orc.prepare(vis_mult=1, imu_mult=1)
    else:
        orc.set_options(calibrate_imu=False); orc.prepare(vis_mult=1)
    lay = orc.layout()
    df, D0 = lay["df"], lay["D"]
    D = D0 + 9 * len(seps)
    for r, res in enumerate(ranks):
        assert (res["lo"], res["hi"]) == frame_shard(N, r, P)
        assert res["n_frames"] == res["hi"] - res["lo"]
        assert res["D"] == case["D"] == D, (r, res["D"], case["D"], D)
        if vi:
            print(f"rank {r}: frames [{res['lo']}, {res['hi']}), pass paths {res['paths']}")
            for k, v in (case["paths"] or {}).items():
                assert res["paths"][k] == v, (r, k, res["paths"])
            assert res["n_blocks"] == res["hi"] - res["lo"] - 1 + (1 if r + 1 < P else 0), (r, res["n_blocks"])
            assert res["W"].shape == (res["n_blocks"], 9, 9)
    if vi:
        W = np.concatenate([res["W"] for res in ranks])
        assert W.shape == (N - 1, 9, 9)
        one = load_slice(ViCalibrator(0), p, 0, N, case["init"]); set_state(one, case, p)
        one.linearize()
        W1 = one.imu_weights(); one.close()
        np.testing.assert_allclose(W, W1, rtol=1e-12, atol=1e-12 * np.abs(W1).max())
        orc.set_imu_weights(W)
    lin = orc.linearize()
    n = lin["A"].shape[0]
    # the all-reduced reduced system of linearize() against the dense Schur complement of the whole Hessian (separators kept)
    H = ref.dense_hessian(lin, df)
    g = ref._pack(lin["gf"], lin["gs"], n, df)
    interior, reduced = ref.sharded_order(n, D0, seps, df)
    S_ref, g_ref, _, _ = ref.sharded_schur(H, g, interior, reduced)
    # the device's columns with a counterpart (all of them, unless rotation-only frames have 6 unknowns: then a separator's 3 velocity
    # columns have none, and the kernels leave them without equations -- zero rows and columns in S, zero g_red and diag H_ss)
    dcols = ref.device_columns(D0, len(seps), df)
    free = np.setdiff1d(np.arange(D), dcols)
    for r, res in enumerate(ranks):
        assert abs(res["lin"]["cost"] - lin["cost"]) <= 1e-10 * abs(lin["cost"]), (r, res["lin"]["cost"], lin["cost"])
        Sd = res["lin"]["S"]
        np.testing.assert_allclose(Sd[np.ix_(dcols, dcols)], S_ref, rtol=1e-6, atol=1e-8 * np.abs(H[np.ix_(reduced, reduced)]).max())
        np.testing.assert_allclose(res["lin"]["g_red"][dcols], g_ref, rtol=1e-6, atol=1e-8 * np.abs(g[reduced]).max())
        assert not np.any(Sd[free]) and not np.any(Sd[:, free]) and not np.any(res["lin"]["g_red"][free]) and not np.any(res["lin"]["hss_diag"][free])
    T0, v0 = orc.frames()
    cams0 = [orc.camera(c) for c in range(orc.n_cams)]
    imu0 = orc.imu_state()
    worst = 0.0
    for k, radius in enumerate(RADII):
        steps = [res["steps"][k] for res in ranks]
        lam = orc.lm_lambda(radius)
        rr = ref.reference_step(lin, lam, df)
        print(f"radius {radius:g}: n = {rr['n']}, kappa(M~) = {rr['kappa']:.3e}, bound = {rr['rel']:.3e}")
        if radius == 1e0:
            assert rr["rel"] <= 1e-9, "badly chosen case: the heavily damped pass must be well conditioned"
        s = rr["scale"]
        lam_f = lam[:n * 9].reshape(n, 9)
        act_f = rr["active"][:n * df].reshape(n, df).all(axis=1)
        for r, (res, got) in enumerate(zip(ranks, steps)):
            assert abs(got["cost"] - lin["cost"]) <= 1e-10 * abs(lin["cost"])
            # damping: the shared parameters, the separators at their columns, the rank's own frames
            np.testing.assert_allclose(got["slam"][:D0], lam[n * 9:], rtol=1e-12)
            for j, f in enumerate(seps):
                np.testing.assert_allclose(got["slam"][D0 + 9 * j:D0 + 9 * j + df], lam_f[f][:df], rtol=1e-12, err_msg=f"separator frame {f}")
            # columns without equations: diag H_ss = 0, Jacobi scale 1, the diagonal clamped to 1e-6 (lm_clamped_diag): damping 1e-6 / radius
            np.testing.assert_allclose(got["slam"][free], 1e-6 / radius, rtol=1e-15)
            assert not np.any(got["delta_s"][free]), got["delta_s"][free]
            lo, hi = res["lo"], res["hi"]
            a = act_f[lo:hi].copy()
            if lo in seps:
                a[0] = False            # (a separator is damped as a column of the reduced system: slam above, not frame_lam)
            assert got["frame_lam"].shape == (hi - lo, 9)
            np.testing.assert_allclose(got["frame_lam"][a, :df], lam_f[lo:hi][a, :df], rtol=1e-12)
        # every rank solves the identical reduced system: delta_s and the shared trial state are the same bits everywhere
        for r in range(1, P):
            np.testing.assert_array_equal(steps[r]["delta_s"], steps[0]["delta_s"], err_msg=f"delta_s of rank {r}")
            np.testing.assert_array_equal(steps[r]["cams"], steps[0]["cams"], err_msg=f"camera trial state of rank {r}")
            np.testing.assert_array_equal(steps[r]["imus"], steps[0]["imus"], err_msg=f"IMU trial state of rank {r}")
        # delta_s against the reference, shared part and separator part
        ds_ref, ss = ref.to_sharded(rr, seps)
        xn = ref.scaled_norm(rr, rr["dfv"], rr["dsv"])
        E = rr["rel"] * xn
        e = (steps[0]["delta_s"][dcols] - ds_ref) / ss
        for what, part in (("shared", e[:D0]), ("separators", e[D0:])):
            ep = float(np.linalg.norm(part))
            assert ep <= E, f"delta_s ({what}): scaled error {ep / xn:.3e} of the step > bound {rr['rel']:.3e}"
            if radius == 1e0 and E > 0:
                worst = max(worst, ep / E)
        print(f"  |delta_s error|~ / |x~_ref| = {np.linalg.norm(e) / xn:.3e}")
        # trial state against the oracle's update with the reference step
        orc.apply_step(rr["dfv"], rr["dsv"])
        T1, v1 = orc.frames()
        cams1 = [orc.camera(c) for c in range(orc.n_cams)]
        imu1 = orc.imu_state()
        ratios = []
        for res, got in zip(ranks, steps):
            lo, hi = res["lo"], res["hi"]
            for f in range(lo, hi):
                sf = s[f * df:(f + 1) * df]
                ratios.append(_block_check(f"frame {f} pose", got["poses"][f - lo], T1[f], T0[f], sf[:6].max(), E))
                if df == 9:
                    ratios.append(_block_check(f"frame {f} velocity", got["vels"][f - lo], v1[f], v0[f], sf[6:9].max(), E))
        ssh = s[n * df:]
        got = steps[0]
        for c in range(orc.n_cams):
            cols = [lay["cam"][c][0] + q for q in range(3)] if lay["cam"][c][0] >= 0 else []
            cols += [lay["cam"][c][1] + q for q in range(3)] if lay["cam"][c][1] >= 0 else []
            nk = len(cams1[c][0])
            cols += [lay["cam"][c][2] + q for q in range(nk)] if lay["cam"][c][2] >= 0 else []
            smax = ssh[cols].max() if cols else 0.0
            ratios.append(_block_check(f"camera {c} T_ck", got["cams"][c][:7], cams1[c][1], cams0[c][1], smax, E))
            ratios.append(_block_check(f"camera {c} intrinsics", got["cams"][c][7:7 + nk], cams1[c][0], cams0[c][0], smax, E))
        if vi:
            b1, sf1, g1, t1 = imu1
            b0, sf0, g0, t0 = imu0
            for what, off, dev, want, x0 in (("gravity", lay["g"], got["imus"][0:2], g1, g0), ("biases", lay["b"], got["imus"][2:8], b1, b0),
                                             ("scale factors", lay["sf"], got["imus"][8:14], sf1, sf0), ("time offset", lay["toff"], got["imus"][14:15], [t1], [t0])):
                smax = ssh[off:off + len(want)].max() if off >= 0 else 0.0
                ratios.append(_block_check(what, dev, want, x0, smax, E))
        if radius == 1e0:
            worst = max([worst] + ratios)
            kappa1, bound1 = rr["kappa"], rr["rel"]
        for f in range(n):
            orc.set_frame(f, T0[f], v0[f])
        for c in range(orc.n_cams):
            orc.set_camera(c, cams0[c][0], cams0[c][1])
        orc.set_imu_state(imu0[0], imu0[1], imu0[2], imu0[3])
    print(f"RESULT {name}: P = {P}, D = {D}, radius 1: kappa(M~) = {kappa1:.3e}, bound = {bound1:.3e}, largest error / bound = {worst:.3e}")


# ---- the read-out contract of a rank that keeps a ghost ---------------------------------------------------------------------------

def check_readouts(store):
    """The four frame- and block-indexed read-outs, called through the C ABI on every rank of a 3-rank visual-inertial split: each
    buffer has its documented size plus PAD sentinel doubles, none of which may change."""
    import ctypes as C
    from vicalib_amd.lib import ViCalibrator, _check
    case = _i(("kb4",), 30, 3, 47)
    P, N = 3, case["n"]
    p = problem(case)

    def buf(n):
        a = np.zeros(n + PAD); a[n:] = SENTINEL
        return a

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def intact(what, a, n):
        assert np.all(a[n:] == SENTINEL), f"{what}: {int(np.sum(a[n:] != SENTINEL))} of the {PAD} doubles past its {n} were written"

    def body(rank):
        group = make_group(store, rank, P)
        lo, hi = frame_shard(N, rank, P)
        cal = load_slice(ViCalibrator(0), p, lo, hi, False)
        set_state(cal, case, p)
        attach(cal, group, rank, P)
        L, h = cal.L, cal.h
        cal.prepare()
        n, D, nc = L.vc_num_frames(h), cal.shared_dim(), cal.NumCameras()
        nb = L.vc_num_imu_blocks(h)
        assert n == hi - lo and D == case["D"]
        assert nb == n - 1 + (1 if rank + 1 < P else 0), (rank, nb)
        cost = C.c_double(0)
        Hpp, gp, S, gr, hd, gs = buf(36 * n), buf(6 * n), buf(D * D), buf(D), buf(D), buf(D)
        _check(L.vc_linearize(h, C.byref(cost), ptr(Hpp), ptr(gp), ptr(S), ptr(gr), ptr(hd), ptr(gs)), "vc_linearize")
        for what, a, k in (("vc_linearize Hpp", Hpp, 36 * n), ("vc_linearize gp", gp, 6 * n), ("vc_linearize S", S, D * D),
                           ("vc_linearize g_red", gr, D), ("vc_linearize hss_diag", hd, D), ("vc_linearize g_s", gs, D)):
            intact(what, a, k)
        Wb = buf(81 * nb)
        _check(L.vc_get_imu_weights(h, ptr(Wb)), "vc_get_imu_weights")
        intact("vc_get_imu_weights", Wb, 81 * nb)
        Hb, gb, cb = buf(1089 * nb), buf(33 * nb), buf(nb)
        _check(L.vc_get_imu_blocks(h, ptr(Hb), ptr(gb), ptr(cb)), "vc_get_imu_blocks")
        for what, a, k in (("vc_get_imu_blocks H", Hb, 1089 * nb), ("vc_get_imu_blocks g", gb, 33 * nb), ("vc_get_imu_blocks cost", cb, nb)):
            intact(what, a, k)
        ds, sl, fl, T, v, cams, imus = buf(D), buf(D), buf(9 * n), buf(7 * n), buf(3 * n), buf(17 * nc), buf(15)
        _check(L.vc_step_hold(h, C.c_double(1e4), C.byref(cost), ptr(ds), ptr(sl), ptr(fl), ptr(T), ptr(v), ptr(cams), ptr(imus)), "vc_step_hold")
        for what, a, k in (("vc_step_hold delta_s", ds, D), ("vc_step_hold slam", sl, D), ("vc_step_hold frame_lam", fl, 9 * n),
                           ("vc_step_hold poses", T, 7 * n), ("vc_step_hold vels", v, 3 * n), ("vc_step_hold cams", cams, 17 * nc),
                           ("vc_step_hold imus", imus, 15)):
            intact(what, a, k)
        group.barrier().wait()
        cal.close()
        return dict(lo=lo, hi=hi, W=Wb[:81 * nb].reshape(nb, 9, 9), H=Hb[:1089 * nb].reshape(nb, 33, 33), g=gb[:33 * nb].reshape(nb, 33), c=cb[:nb])

    ranks = run_ranks(P, body)
    one = load_slice(ViCalibrator(0), p, 0, N, False); set_state(one, case, p)
    one.linearize()
    W1 = one.imu_weights(); H1, g1, c1 = one.imu_blocks()
    one.close()
    for r, res in enumerate(ranks):
        lo, hi = res["lo"], res["hi"]
        blocks = range(lo, hi if r + 1 < P else hi - 1)          # the block that ends in the ghost (global index hi - 1) included
        for what, got, want in (("weights", res["W"], W1), ("H", res["H"], H1), ("g", res["g"], g1), ("cost", res["c"], c1)):
            np.testing.assert_allclose(got, want[list(blocks)], rtol=1e-12, atol=1e-12 * np.abs(want).max(), err_msg=f"rank {r}: IMU block {what}")
    print("RESULT readouts: every buffer intact, the ghost-ending blocks match the single-process blocks")


# ---- the width limit of the reduced solve ----------------------------------------------------------------------------------------

def check_limit(store):
    """D = 180 is refused by every rank's upload with VC_ERR_UNSUPPORTED; the same calibrators then take a small problem."""
    from vicalib_amd.lib import ViCalibrator, VicalibError
    P = 8
    big = _i(LIMIT_MODELS, 24, P, 180)
    small = _i(("kb4",), 16, P, 92)
    pb, ps = problem(big), problem(small)

    def body(rank):
        group = make_group(store, rank, P)
        lo, hi = frame_shard(big["n"], rank, P)
        cal = load_slice(ViCalibrator(0), pb, lo, hi, False)
        set_state(cal, big, pb)
        attach(cal, group, rank, P)
        try:
            cal.prepare()
        except VicalibError as e:
            assert "VC_ERR_UNSUPPORTED" in str(e), str(e)
        else:
            raise AssertionError(f"rank {rank}: a reduced system of D = {cal.shared_dim()} was accepted")
        cal.Clear()
        lo, hi = frame_shard(small["n"], rank, P)
        load_slice(cal, ps, lo, hi, False)
        set_state(cal, small, ps)
        attach(cal, group, rank, P)
        lin = cal.linearize()
        assert cal.shared_dim() == small["D"], cal.shared_dim()
        got = cal.step_hold(1e4)
        group.barrier().wait()
        cal.close()
        return dict(cost=lin["cost"], ds=got["delta_s"])

    ranks = run_ranks(P, body)
    one = load_slice(ViCalibrator(0), ps, 0, small["n"], False); set_state(one, small, ps)
    c1 = one.linearize()["cost"]; one.close()
    for r, res in enumerate(ranks):
        assert abs(res["cost"] - c1) <= 1e-10 * abs(c1), (r, res["cost"], c1)
        np.testing.assert_array_equal(res["ds"], ranks[0]["ds"])
        assert np.all(np.isfinite(res["ds"])) and np.any(res["ds"] != 0)
    print("RESULT limit: D = 180 refused on every rank, D = 92 solved afterwards")


if __name__ == "__main__":
    what, store_dir = sys.argv[1], sys.argv[2]
    store = os.path.join(store_dir, "store_" + what)
    try:
        if what == "readouts":
            check_readouts(store)
        elif what == "limit":
            check_limit(store)
        else:
            check_case(what, store)
    except BaseException as e:      # noqa: BLE001
        print("WORKER-FAILURE %s: %s\n%s" % (what, type(e).__name__, (str(e) + "\n" + traceback.format_exc())[:6000]), flush=True)
        os._exit(1)
    print("ok", what, flush=True)
    os._exit(0)
