"""GPU tier of the collision audit and the closed loop's collision stop at their lane-layout edges: the plan audit at every
segment width (N + 1 from 2 to past 64, strided walks with a ragged last pass, partial last blocks), per-stage rows and
variant 4's stage-0 rows, exact ties inside a lane and across lanes, the NaN contract; the rollout audit at max_steps 1 to
96 (several intervals per lane), n_sub 1 to 1024, right after reset and on failed rollouts, against the host build of the
same core fed with the device's own history; the stop's wave reduction at n_sub 1 to 63, sampled and certified, fused
and lock-step, and the audit of a stopped run."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import kkt_check
from tests import test_audit_core as core
from tests import test_rollout_stop_core as stop_core
from tests.test_gpu_audit import _distances, _knot_boxes
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import DeviceRollouts, pack_worlds, rollout_dims
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.scenarios import DMIN, EGO, make_world_c5

pytestmark = pytest.mark.gpu
HIST = ("x_closed", "u_closed", "T_closed", "x_openloop", "variant", "iters", "status", "dyn", "steps", "flags")


@pytest.fixture(scope="module")
def ahost():
    return core.load_host()


@pytest.fixture(scope="module")
def shost():
    return stop_core.load_host()


def _np(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ plans
def _gpu_plan(x, A, b, m, variant, per_stage=True):
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_clearance
    return _np(plan_clearance(x, A, b, m, ego=EGO, variant=variant, per_stage=per_stage))


# (N, B, n_obs): every segment width (N + 1 = 2, 3, 7, 8, 32, 64), the strided walk (75, 201) with a ragged last pass,
# the full wave (64); B = 257 leaves the last 256-thread block partial
PLAN_SHAPES = [(1, 257, 3), (2, 3, 8), (6, 257, 8), (7, 1, 1), (31, 257, 1), (63, 3, 3), (63, 257, 8), (64, 257, 3),
               (74, 257, 8), (74, 3, 1), (200, 257, 3), (200, 1, 8)]


@pytest.mark.parametrize("N,B,n_obs", PLAN_SHAPES)
def test_plan_audit_at_every_segment_width(ahost, N, B, n_obs):
    rng = np.random.default_rng(1000 * N + 10 * B + n_obs)
    m = core.PLAN_M[n_obs]
    x, A, b, variant, ties = core.random_plans(rng, B, N, n_obs)
    au = _gpu_plan(x, A, b, m, variant)
    so = au["stage_obst"]
    # every instance against the host build of the reduction, a sample of them against kkt_check.polytope_distance
    hmc, hst, hob, hso = core.host_plan_clearance(ahost, x, A, b, m, variant)
    assert np.abs(so - hso).max() <= 1e-9
    idx = sorted({0, B // 2, B - 2, B - 1} & set(range(B)))
    ref = core.numpy_stage_obst(x, A, b, m, variant, idx)
    assert np.abs(so[idx] - ref).max() <= 1e-9
    assert (ref < 0).any() and (ref > 0).any()
    assert (so < 0).any() and (so > 0).any()
    assert np.abs(au["min_clear"] - hmc).max() <= 1e-9
    # the minimum and its (stage, obstacle) exactly, from the device's own per-pair words
    v, s, o = core.first_argmin(so)
    assert np.array_equal(au["min_clear"], v) and np.array_equal(au["arg_stage"], s) and np.array_equal(au["arg_obst"], o)
    n_tie = 0
    for i, t in enumerate(ties):
        if t is not None and au["min_clear"][i] == so[i, t[0]].min():
            assert au["arg_stage"][i] == t[0], (i, t, au["arg_stage"][i])
            n_tie += 1
    assert n_tie >= min(B // 2, 1) * (N + 1 > 1)
    # per_stage off: the same words
    au0 = _gpu_plan(x, A, b, m, variant, per_stage=False)
    for k in ("min_clear", "arg_stage", "arg_obst"):
        assert np.array_equal(au0[k].view(np.uint8), au[k].view(np.uint8)), k


def test_plan_audit_ties_inside_a_lane_and_across_lanes():
    """N + 1 = 64 (one stage per lane): stages 3 and 40 tie across lanes; N + 1 = 75 (seg 64): stages 3 and 67 share lane
    3; obstacle 0 and its copy tie within every lane"""
    for N, s0, s1 in ((63, 3, 40), (74, 3, 67), (74, 10, 70), (200, 5, 133)):
        rng = np.random.default_rng(N + s1)
        m = core.PLAN_M[8]
        x, A, b, variant, _ = core.random_plans(rng, 64, N, 8)
        o4 = sum(m[:4])                                                     # the row of obstacle 4
        A[:, :, o4], b[:, :, o4] = A[:, :, 0], b[:, :, 0]                   # obstacle 4 = half-plane 0 everywhere
        variant[:] = np.where(variant == 4, 0, variant)
        for i in range(len(x)):
            a, bb = A[i, s0, 0], b[i, s0, 0]
            x[i, :2, s0] = a * bb / (a @ a) - 40.0 * a / np.linalg.norm(a)
            x[i, :, s1], A[i, s1], b[i, s1] = x[i, :, s0], A[i, s0], b[i, s0]
        au = _gpu_plan(x, A, b, m, variant)
        so = au["stage_obst"]
        hit = au["min_clear"] == so[:, s0, 0]
        assert hit.sum() >= 16
        assert (so[hit, s1, 0] == so[hit, s0, 0]).all() and (so[hit, s0, 4] == so[hit, s0, 0]).all()
        assert (au["arg_stage"][hit] == s0).all() and (au["arg_obst"][hit] == 0).all(), N


def test_plan_audit_variant_4_reads_stage_0_rows():
    rng = np.random.default_rng(44)
    for N, n_obs in ((6, 8), (74, 3)):
        m = core.PLAN_M[n_obs]
        x, A, b, variant, _ = core.random_plans(rng, 257, N, n_obs)
        au = _gpu_plan(x, A, b, m, variant)
        b2 = b.copy()
        b2[:, 1:] -= 3.0
        au2 = _gpu_plan(x, A, b2, m, variant)
        v4 = variant == 4
        assert v4.sum() > 20 and (~v4).sum() > 20
        for k in ("min_clear", "arg_stage", "arg_obst", "stage_obst"):
            assert np.array_equal(au2[k][v4], au[k][v4]), k
        assert (au2["stage_obst"][~v4][:, 1:] != au["stage_obst"][~v4][:, 1:]).all()
        # variant None: every stage against its own rows, as variant 0
        v0 = np.zeros_like(variant)
        aun, au0 = _gpu_plan(x, A, b, m, None), _gpu_plan(x, A, b, m, v0)
        for k in aun:
            assert np.array_equal(aun[k].view(np.uint8), au0[k].view(np.uint8)), k
        ref = core.numpy_stage_obst(x, A, b, m, None, [0, 1, 255, 256])
        assert np.abs(aun["stage_obst"][[0, 1, 255, 256]] - ref).max() <= 1e-9


@pytest.mark.parametrize("N", [7, 74])
def test_plan_audit_nan_contract(ahost, N):
    """NaN / infinite poses and NaN rows measure NaN, min_clear is NaN at the first such pair; the finite instances of the
    batch give the words of a run without the others"""
    rng = np.random.default_rng(9 + N)
    m = core.PLAN_M[3]
    x, A, b, variant, B0, bad = core.nan_plans(rng, N=N)
    au = _gpu_plan(x, A, b, m, variant)
    for j, pairs in enumerate(bad):
        i = B0 + j
        got = {(int(k), int(o)) for k, o in zip(*np.nonzero(np.isnan(au["stage_obst"][i])))}
        assert got == pairs, (j, got)
        assert np.isnan(au["min_clear"][i])
        assert (au["arg_stage"][i], au["arg_obst"][i]) == min(pairs), j
    fin = _gpu_plan(x[:B0], A[:B0], b[:B0], m, variant[:B0])
    for k in fin:
        assert np.array_equal(au[k][:B0].view(np.uint8), fin[k].view(np.uint8)), k
    hmc, hst, hob, _ = core.host_plan_clearance(ahost, x, A, b, m, variant)
    assert np.array_equal(np.isnan(hmc), np.isnan(au["min_clear"]))
    assert np.array_equal(hst[B0:], au["arg_stage"][B0:]) and np.array_equal(hob[B0:], au["arg_obst"][B0:])


# ------------------------------------------------------------------------------------------------ rollouts
def host_audit(shost, w, o, N, S, n_sub, sel=None):
    """rollout_stop_host_audit on the device history o of worlds w (rollouts sel): step_min, lower [B,S], first_collision"""
    sel = np.arange(w.batch) if sel is None else np.asarray(sel)
    ws = w.slice(int(sel[0]), int(sel[-1]) + 1) if len(sel) == sel[-1] - sel[0] + 1 else None
    assert ws is not None, "a contiguous range"
    d = rollout_dims(ws, N, S)
    B = ws.batch
    c = lambda a: np.ascontiguousarray(a[sel])
    ins = stop_core._inputs(ws)
    step_min, lower, fc = np.zeros((B, S)), np.zeros((B, S)), np.zeros(B, np.int32)
    xc, Tc, dh, st, fl = c(o["x_closed"]), c(o["T_closed"]), c(o["dyn"]), c(o["steps"]), c(o["flags"])
    rc = shost.rollout_stop_host_audit(ctypes.byref(d), _p(ins[4]), _p(ins[5]), _p(ins[6]), _p(np.asarray(EGO, float)),
                                       _p(xc), _p(Tc), _p(dh), _p(st), _p(fl), int(n_sub), _p(step_min), _p(lower), _p(fc))
    assert rc == 0
    return step_min, lower, fc


def single_knot(ahost, w, o, b):
    """the audit of a rollout without steps: knot 0 alone (audit_host_interval with n_sub = 0): (value, obstacle)"""
    Ms = w.static_A.shape[1]
    kb = _knot_boxes(w, o, b)[:1]
    dyn = np.ascontiguousarray(w.dyn[b] if w.n_dyn else np.zeros((0, 13)))
    scene = (np.ascontiguousarray(w.static_A[b].reshape(Ms, 2)), np.ascontiguousarray(w.static_b[b].reshape(Ms)),
             np.asarray(w.m_static, np.int32), dyn)
    p = o["x_closed"][b, 0]
    out = core._interval(ahost, scene, p, p, kb[0], kb[0], 0)
    return out[0], int(out[4])


def interval_arg(ahost, w, o, b, s, n_sub):
    """(value, obstacle) of interval s of rollout b from the host core"""
    Ms = w.static_A.shape[1]
    kb = _knot_boxes(w, o, b)
    dyn = np.ascontiguousarray(w.dyn[b] if w.n_dyn else np.zeros((0, 13)))
    scene = (np.ascontiguousarray(w.static_A[b].reshape(Ms, 2)), np.ascontiguousarray(w.static_b[b].reshape(Ms)),
             np.asarray(w.m_static, np.int32), dyn)
    out = core._interval(ahost, scene, o["x_closed"][b, s], o["x_closed"][b, s + 1], kb[s], kb[s + 1], n_sub)
    return out[0], int(out[4])


def knot_distances(w, o, b, c5=True):
    """[steps+1] smallest distance at the knots: C5 through test_gpu_audit._distances, other worlds (wedges) through
    kkt_check.polytope_distance"""
    steps = int(o["steps"][b])
    poses, boxes = o["x_closed"][b, :steps + 1], _knot_boxes(w, o, b)
    if c5:
        return _distances(w, b, poses, boxes)
    off = np.concatenate([[0], np.cumsum(w.m_static)]).astype(int)
    A, bb = w.static_A[b].reshape(-1, 2), w.static_b[b].reshape(-1)
    out = np.full(len(poses), np.inf)
    for k, pz in enumerate(poses):
        car = kkt_check.car_corners(pz, EGO)
        for i in range(len(w.m_static)):
            out[k] = min(out[k], kkt_check.polytope_distance(car, A[off[i]:off[i + 1]], bb[off[i]:off[i + 1]]))
        for j in range(w.n_dyn):
            if boxes[k, j, 2] > 0:
                info = w.dyn[b, j]
                V = stop_core.rect_vertices(boxes[k, j, 0], boxes[k, j, 1], info[11], info[12], info[3], info[4])
                rows = [stop_core.edge_row(*V[e], *V[(e + 1) % 4]) for e in range(4)]
                out[k] = min(out[k], kkt_check.polytope_distance(car, np.array([r[0] for r in rows]), np.array([r[1] for r in rows])))
    return out


def check_rollout_audit(ahost, shost, w, dr, o, N, n_sub, sub=None, c5=True):
    """the device audit at n_sub against the host core fed with the device's own history o (rollouts sub, a prefix)"""
    S = dr.max_steps
    au = _np(dr.audit(n_sub, per_step=True))
    B = w.batch if sub is None else sub
    hs, hl, hfc = host_audit(shost, w, o, N, S, n_sub, np.arange(B))
    steps, flags = o["steps"][:B], o["flags"][:B]
    sm = au["step_min"][:B]
    for b in range(B):
        st = int(steps[b])
        n_int = max(st, 1)
        assert np.isinf(sm[b, n_int:]).all() and (sm[b, n_int:] > 0).all(), b
        if st == 0:
            v, ob = single_knot(ahost, w, o, b)
            assert abs(sm[b, 0] - v) <= 1e-12 and au["lower_bound"][b] == sm[b, 0], b
            assert au["arg_obst"][b] == ob and au["arg_step"][b] == 0, b
            assert au["first_collision"][b] == (0 if v < 0 else -1), b
            continue
        assert np.abs(sm[b, :st] - hs[b, :st]).max() <= 1e-12, b
        assert abs(au["lower_bound"][b] - hl[b, :st].min()) <= 1e-12, b
        if not (np.abs(hs[b, :st]) <= 1e-12).any():
            assert au["first_collision"][b] == hfc[b], b
        s_arg = int(np.argmin(sm[b]))
        assert au["min_clear"][b] == sm[b, s_arg] and au["arg_step"][b] == s_arg, b
    # the obstacle of the minimum, and the knots, on a sample (one host interval, numpy distances per rollout)
    for b in list(range(min(B, 12))) + [B - 1]:
        st = int(steps[b])
        if st:
            v, ob = interval_arg(ahost, w, o, b, int(au["arg_step"][b]), n_sub)
            assert abs(v - au["min_clear"][b]) <= 1e-12 and au["arg_obst"][b] == ob, b
        kd = knot_distances(w, o, b, c5)
        viol = np.flatnonzero(kd < DMIN - 1e-6)
        near = (np.abs(kd - (DMIN - 1e-6)) <= 1e-9).any()
        if not near:
            assert au["first_violation"][b] == (viol[0] if len(viol) else -1), b
    assert (au["lower_bound"] <= au["min_clear"]).all()
    return au


@pytest.mark.parametrize("S,n_dyn,n_subs", [(1, 2, (1, 64)), (2, 1, (2, 63)), (30, 4, (1, 63)), (64, 0, (2, 64)),
                                            (96, 2, (1, 63, 64))])
def test_rollout_audit_at_every_max_steps(ahost, shost, S, n_dyn, n_subs):
    w = pack_worlds([make_world_c5(i, n_dyn=n_dyn) for i in range(256)])
    dr = DeviceRollouts(w, N=5, max_steps=S)
    try:
        # straight after reset: every rollout is a single knot
        o0 = _np(dr.read())
        assert (o0["steps"] == 0).all()
        check_rollout_audit(ahost, shost, w, dr, o0, 5, 8)
        dr.run()
        o = _np(dr.read())
        if S > 64:
            assert (o["steps"] > 64).any()
        if S >= 30 and n_dyn:
            assert (o["flags"] == _lib.DONE_FAILED).any()
        for n_sub in n_subs:
            check_rollout_audit(ahost, shost, w, dr, o, 5, n_sub)
        # n_sub = 1024 on a prefix; soundness of the certified bound on the device, every rollout
        fine = check_rollout_audit(ahost, shost, w, dr, o, 5, 1024, sub=64)
        for n_sub in (1, 2, 4, 63):
            lb = _np(dr.audit(n_sub))["lower_bound"]
            assert (lb <= fine["min_clear"] + 1e-12).all(), n_sub
    finally:
        dr.close()


def test_rollout_audit_on_demo9_past_64_steps(ahost, shost):
    """the reference's demo9 (wedge walls, one moving box) for 96 steps: more than 64 intervals, several per lane"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.demo_setting import problemSetting
    w = pack_worlds(copy.deepcopy([problemSetting("demo9")]))
    dr = DeviceRollouts(w, max_steps=96)
    try:
        dr.run()
        o = _np(dr.read())
        assert o["steps"][0] > 64, o["steps"]
        for n_sub in (1, 2, 63, 64, 1024):
            check_rollout_audit(ahost, shost, w, dr, o, dr.N, n_sub, c5=False)
    finally:
        dr.close()


# ------------------------------------------------------------------------------------------------ collision stop
def _run(w, mode, **kw):
    dr = DeviceRollouts(w, N=5, **kw)
    if mode == "lockstep":
        dr.set_mode("lockstep")
        for _ in range(dr.max_steps):
            dr.step()
    else:
        dr.run()
    return dr, _np(dr.read())


STOP_WORLDS = [(1024, 2), (256, 0), (256, 4)]


@pytest.mark.parametrize("B,n_dyn", STOP_WORLDS)
def test_stop_wave_at_every_n_sub(shost, B, n_dyn):
    w = pack_worlds([make_world_c5(i, n_dyn=n_dyn) for i in range(B)])
    dr_off, off = _run(w, "fused")
    S = dr_off.max_steps
    st_off = off["steps"]
    n_stopped = 0
    for n_sub in (1, 2, 32, 63):
        hs, hl, _ = host_audit(shost, w, off, 5, S, n_sub)
        au_off = _np(dr_off.audit(n_sub, per_step=True))
        for mode in ("fused", "lockstep"):
            for cert in (0, 1):
                want = hl if cert else hs
                # never stopping: the unstopped history, every interval measured as the host audit measures it
                dr, never = _run(w, mode, collision_stop={"n_sub": n_sub, "clearance": -1e9, "certified": bool(cert)})
                dr.close()
                for k in HIST:
                    assert np.array_equal(never[k], off[k]), (n_sub, mode, cert, k)
                clr = never["clearance"]
                for b in range(B):
                    k = int(st_off[b])
                    assert np.abs(clr[b, :k] - want[b, :k]).max(initial=0.0) <= 1e-12, (n_sub, mode, cert, b)
                    assert np.isinf(clr[b, k:]).all(), (n_sub, mode, cert, b)
                # a real threshold: the first interval below it ends the rollout
                thr = DMIN if cert else 0.0
                dr, on = _run(w, mode, collision_stop={"n_sub": n_sub, "clearance": thr, "certified": bool(cert)})
                au_on = _np(dr.audit(n_sub, per_step=True))
                dr.close()
                for b in range(B):
                    k_off = int(st_off[b])
                    below = np.flatnonzero(want[b, :k_off] < thr)
                    k = int(on["steps"][b])
                    if not (np.abs(want[b, :k_off] - thr) <= 1e-12).any():
                        assert (on["flags"][b] == _lib.DONE_COLLISION) == (len(below) > 0), (n_sub, mode, cert, b)
                        assert k == (below[0] + 1 if len(below) else k_off), (n_sub, mode, cert, b)
                        if not len(below):
                            assert on["flags"][b] == off["flags"][b], (n_sub, mode, cert, b)
                    assert np.array_equal(on["x_closed"][b, :k + 1], off["x_closed"][b, :k + 1]), (n_sub, mode, cert, b)
                    assert np.array_equal(on["clearance"][b, :k], clr[b, :k]), (n_sub, mode, cert, b)
                    # the audit of the stopped run: the update law reproduces the record of the unstopped one
                    if k:
                        assert np.array_equal(au_on["step_min"][b, :k], au_off["step_min"][b, :k]), (n_sub, mode, cert, b)
                        fc = int(au_off["first_collision"][b])
                        assert au_on["first_collision"][b] == (fc if 0 <= fc < k else -1), (n_sub, mode, cert, b)
                n_stopped += int((on["flags"] == _lib.DONE_COLLISION).sum())
    dr_off.close()
    assert n_stopped > 0


# ------------------------------------------------------------------- the plan calls' batch: refusals, wrapper = C call
PAD = 32                          # sentinel words on either side of every output
SENT_F, SENT_I = -777.25, -777
CLEARANCE_OUTS = (("min_clear", torch.float64), ("arg_stage", torch.int32), ("arg_obst", torch.int32), ("stage_obst", torch.float64))


def _dev_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded_clearance(B, N1, n_obs):
    """every output of obca_plan_clearance in the middle of a buffer of sentinels: name -> (buffer, view of the output)"""
    out = {}
    for name, dt in CLEARANCE_OUTS:
        n = B * N1 * n_obs if name == "stage_obst" else B
        buf = torch.full((n + 2 * PAD,), SENT_F if dt == torch.float64 else SENT_I, dtype=dt, device="cuda")
        out[name] = (buf, buf[PAD:PAD + n])
    return out


def _sentinels(g, inner):
    torch.cuda.synchronize()
    for name, (buf, view) in g.items():
        s = SENT_F if buf.dtype == torch.float64 else SENT_I
        assert (buf[:PAD] == s).all() and (buf[-PAD:] == s).all(), name
        assert bool((view == s).all()) if inner else not (view == s).any(), name


def _raw_clearance(g, c, **over):
    """obca_plan_clearance itself on the device tensors of c, outputs into the guarded buffers g; `over` replaces
    arguments of the C call by name"""
    from tests.test_plan_batch_core import batch_args
    own = dict({k: _dev_ptr(v[1]) for k, v in g.items()}, device=torch.cuda.current_device())
    own.update({k: over.pop(k) for k in list(over) if k in own})
    return _lib.load().obca_plan_clearance(*batch_args(c, _dev_ptr, **over), *[own[k] for k, _ in CLEARANCE_OUTS], own["device"],
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.fixture(scope="module")
def small():
    from tests.test_plan_batch_core import small_batch
    c = small_batch()
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    return c, dict(x=t(c["x"]), A=t(c["A"]), b=t(c["b"]), m=c["m"], variant=t(c["variant"], torch.int32))


def _refusals():
    from tests.test_plan_batch_core import REFUSALS
    return REFUSALS + [dict(min_clear=None), dict(arg_stage=None), dict(arg_obst=None), dict(device=-1)]


@pytest.mark.parametrize("bad", _refusals(), ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_refused_plan_clearance_leaves_every_output_alone(small, bad):
    """the batch's refusal table (tests/test_plan_batch_core.py) and obca_plan_clearance's own pointers through the C ABI:
    host-side checks only, the call returns before it touches the device"""
    c, dev = small
    dev = dict(dev, variant=None)
    g = _guarded_clearance(5, 4, 3)
    assert _raw_clearance(g, dev, **bad) == core.E_INVAL
    _sentinels(g, inner=True)
    assert _raw_clearance(g, dev) == 0                                         # and the same call, unchanged, runs
    _sentinels(g, inner=False)


@pytest.mark.parametrize("inputs", ["torch", "numpy"])
def test_plan_wrappers_equal_the_c_calls(small, inputs):
    """audit.plan_clearance (no variant) and audit.plan_sweep (variants 4, 6, 8, 0, 6) against the raw C calls, word for word,
    from device tensors and from numpy arrays"""
    from tests import test_gpu_plan_sweep as gsweep
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.audit import plan_clearance, plan_sweep
    c, dev = small
    src = dev if inputs == "torch" else c
    words = lambda t: t.contiguous().reshape(-1).view(torch.uint8).cpu()
    g = _guarded_clearance(5, 4, 3)
    assert _raw_clearance(g, dict(dev, variant=None)) == 0
    _sentinels(g, inner=False)
    got = plan_clearance(src["x"], src["A"], src["b"], c["m"], ego=core.EGO, per_stage=True)
    assert sorted(got) == sorted(k for k, _ in CLEARANCE_OUTS)
    for k, _ in CLEARANCE_OUTS:
        assert torch.equal(words(got[k]), words(g[k][1])), k
    gs = gsweep._guarded(5, 3)
    assert gsweep.raw_call(gs, (dev["x"], dev["A"], dev["b"], dev["variant"]), c["m"], n_sub=16) == 0
    gsweep._untouched(gs)
    got = plan_sweep(src["x"], src["A"], src["b"], c["m"], n_sub=16, ego=core.EGO, variant=src["variant"], per_interval=True)
    assert sorted(got) == sorted(gs)
    for k in gs:
        assert torch.equal(words(got[k]), words(gs[k][1])), k
