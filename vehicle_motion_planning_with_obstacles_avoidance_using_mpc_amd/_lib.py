"""ctypes binding of libobca_mpc.so (C ABI in include/obca_mpc.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is visible, loading
or solving raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libobca_mpc.so")

OBCA_MAX_OBST = 8
OBCA_MAX_EDGES = 4


class ObcaDims(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int32), ("n_obs", ctypes.c_int32), ("m", ctypes.c_int32 * OBCA_MAX_OBST),
                ("max_batch", ctypes.c_int32), ("device", ctypes.c_int32)]


class ObcaWeights(ctypes.Structure):
    _fields_ = [("Q", ctypes.c_double * 9), ("P", ctypes.c_double * 9), ("R1", ctypes.c_double * 4),
                ("R2", ctypes.c_double * 4)]


class ObcaParams(ctypes.Structure):
    """obca_params (include/obca_mpc.h).  A new instance is what obca_params_init leaves: all zero (= every default),
    struct_size set."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("time_bound", ctypes.c_uint32),
                ("free_time", ObcaWeights), ("fixed_time", ObcaWeights),
                ("xL", ctypes.c_double * 2), ("xU", ctypes.c_double * 2),
                ("uL", ctypes.c_double * 2), ("uU", ctypes.c_double * 2),
                ("ego", ctypes.c_double * 4), ("dmin", ctypes.c_double),
                ("tol", ctypes.c_double), ("rho", ctypes.c_double), ("feas_tol", ctypes.c_double),
                ("max_iter_free", ctypes.c_int32), ("max_iter_fixed", ctypes.c_int32), ("max_soc", ctypes.c_int32),
                ("start_order", ctypes.c_int32), ("single_start", ctypes.c_int32), ("patience", ctypes.c_int32),
                ("retry_iter", ctypes.c_int32), ("dodge", ctypes.c_int32), ("terminal_screen", ctypes.c_int32)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(ObcaParams)


# obca_params.start_order (include/obca_mpc.h)
START_DEFAULT, START_WINDOW_FIRST, START_ZEROS_FIRST, START_X0_FIRST = 0, 1, 2, 3
START_ORDERS = {"default": START_DEFAULT, "x0": START_X0_FIRST, "window": START_WINDOW_FIRST, "zeros": START_ZEROS_FIRST}
# obca_params.time_bound (include/obca_mpc.h): obca_mpc4's bound on its time scale -- the reference's signed sum, or the window's L1 arc length
TIME_BOUND_REFERENCE, TIME_BOUND_PATH = 0, 1
TIME_BOUNDS = {"reference": TIME_BOUND_REFERENCE, "path": TIME_BOUND_PATH}


class ObcaRolloutDims(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int32), ("n_static", ctypes.c_int32), ("m_static", ctypes.c_int32 * OBCA_MAX_OBST),
                ("n_dyn", ctypes.c_int32), ("path_max", ctypes.c_int32), ("batch", ctypes.c_int32),
                ("max_steps", ctypes.c_int32), ("device", ctypes.c_int32), ("N_fix", ctypes.c_int32)]


# what every obca_*_init writes besides zeros and struct_size (csrc/obca_loop_core.h); a descriptor has those it names
DESCRIPTOR_DEFAULTS = {"clearance": -1e300, "far": 100.0, "goal_tol2": 0.1, "ego": (1.7, 0.75, 1.7, 0.75)}


class Descriptor(ctypes.Structure):
    """The base of the loop-step descriptors of include/obca_mpc.h.  A subclass states its members in header order through
    ``members`` and names its defaults; a new instance is what its obca_*_init leaves: all zero, struct_size set, the named
    words of DESCRIPTOR_DEFAULTS."""
    DEFAULTS = ()

    @staticmethod
    def members(ints, doubles, pointers):
        """_fields_ of a descriptor: struct_size, reserved_, the int32 members, the doubles (``ego`` is double[4]), the pointers"""
        return [("struct_size", ctypes.c_uint32), ("reserved_", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in ints] + \
               [(n, ctypes.c_double * 4 if n == "ego" else ctypes.c_double) for n in doubles] + [(n, ctypes.c_void_p) for n in pointers]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = ctypes.sizeof(type(self))
        self.set(**{n: DESCRIPTOR_DEFAULTS[n] for n in self.DEFAULTS})

    def set(self, **members):
        """scalar members from an int or float, ``ego`` from a 4-sequence, pointer members from None, a torch tensor, a numpy
        array or an integer address"""
        kinds = dict(self._fields_)
        for name, v in members.items():
            if name not in kinds:
                raise AttributeError("%s has no member %r" % (type(self).__name__, name))
            if kinds[name] is ctypes.c_void_p and v is not None:
                v = v.data_ptr() if hasattr(v, "data_ptr") else (v.ctypes.data if hasattr(v, "ctypes") else int(v))
            elif name == "ego":
                v = (ctypes.c_double * 4)(*[float(q) for q in v])
            setattr(self, name, v)
        return self


class ObcaPoolLoop(Descriptor):
    """obca_pool_loop (include/obca_mpc.h), the descriptor of obca_pool_loop_advance.  A new instance is what
    obca_pool_loop_init leaves: all zero, struct_size set, clearance -1e300 (never stops), goal_tol2 0.1, the default ego."""
    _fields_ = Descriptor.members(("B", "K", "E", "N", "n_sel", "path_max", "max_steps", "variant", "n_sub", "reserved2_"),
                                  ("clearance", "goal_tol2", "ego"),
                                  ("pool_A", "pool_v", "goal", "path", "path_len", "status", "iters", "ts_opt", "xopt", "uopt", "sel", "x0",
                                   "u0", "pool_b", "k", "flags", "x_closed", "u_closed", "T_closed", "status_hist", "iters_hist",
                                   "clear_hist", "sel_hist", "xref_out", "variant_out"))
    DEFAULTS = ("clearance", "goal_tol2", "ego")


# obca_fleet.see / obca_fleet.predict (include/obca_mpc.h)
FLEET_SEE_ALL, FLEET_SEE_LOWER = 0, 1
FLEET_SEE = {"all": FLEET_SEE_ALL, "lower": FLEET_SEE_LOWER}
FLEET_PREDICT_VELOCITY, FLEET_PREDICT_STATIC = 0, 1
FLEET_PREDICT = {"velocity": FLEET_PREDICT_VELOCITY, "static": FLEET_PREDICT_STATIC}


class ObcaFleet(Descriptor):
    """obca_fleet (include/obca_mpc.h), the descriptor of obca_fleet_step.  A new instance is what obca_fleet_init leaves: all
    zero (see ALL, predict VELOCITY, margin 0), struct_size set, clearance -1e300 (never stops), far 100, the default ego."""
    _fields_ = Descriptor.members(("G", "V", "Ks", "N", "max_steps", "step", "n_sub", "see", "predict", "reserved2_"),
                                  ("clearance", "margin", "far", "ego"),
                                  ("x_prev", "x0", "u0", "k", "flags", "pool_A", "pool_b", "pool_v", "agent_clear_hist", "xref_out",
                                   "variant_out"))
    DEFAULTS = ("clearance", "far", "ego")


class ObcaFleetTracks(Descriptor):
    """obca_fleet_tracks (include/obca_mpc.h), the descriptor of the call of that name.  A new instance is what
    obca_fleet_tracks_init leaves: all zero (see ALL, margin 0), struct_size set, far 100, the default ego."""
    _fields_ = Descriptor.members(("G", "V", "N", "step", "see", "reserved2_"), ("margin", "far", "ego"),
                                  ("x0", "flags", "k", "xopt", "status", "track_A", "track_b", "track_ok"))
    DEFAULTS = ("far", "ego")


# obca_pool_tracks.predict (include/obca_mpc.h)
TRACK_PREDICT_TRACK, TRACK_PREDICT_VELOCITY, TRACK_PREDICT_STATIC = 0, 1, 2
TRACK_PREDICT = {"track": TRACK_PREDICT_TRACK, "velocity": TRACK_PREDICT_VELOCITY, "static": TRACK_PREDICT_STATIC}


class ObcaPoolTracks(Descriptor):
    """obca_pool_tracks (include/obca_mpc.h), the descriptor of the call of that name.  A new instance is what
    obca_pool_tracks_init leaves: all zero (predict TRACK, margin 0, t0 NULL), struct_size set, clearance -1e300 (never
    stops), far 100, the default ego."""
    _fields_ = Descriptor.members(("B", "K", "Kt", "N", "L", "group", "max_steps", "step", "n_sub", "predict"),
                                  ("clearance", "margin", "far", "ego"),
                                  ("track_x", "track_t", "track_len", "track_size", "t0", "Ts", "x_prev", "x0", "k", "flags", "pool_A",
                                   "pool_b", "pool_v", "stage_A", "stage_b", "stage_ok", "track_state", "track_clear_hist", "xref_out",
                                   "variant_out"))
    DEFAULTS = ("clearance", "far", "ego")


class ObcaPlanTracks(Descriptor):
    """obca_plan_tracks (include/obca_mpc.h), the descriptor of the call of that name.  A new instance is what
    obca_plan_tracks_init leaves: all zero (t0, x0, variant, status and score NULL), struct_size set, far 100, the default ego."""
    _fields_ = Descriptor.members(("B", "K", "Kt", "N", "L", "group", "n_sub", "reserved2_"), ("far", "ego"),
                                  ("track_x", "track_t", "track_len", "track_size", "t0", "dt", "x", "x0", "variant", "status", "score",
                                   "track_clear", "track_min", "track_state"))
    DEFAULTS = ("far", "ego")


EXPORTS = ("obca_create", "obca_destroy", "obca_solve_batch", "obca_lds_bytes", "obca_strerror", "obca_version", "obca_params_init",
           "obca_set_profile_buffer", "obca_set_mode", "obca_set_two_sided_sweep", "obca_rollouts_create", "obca_rollouts_destroy", "obca_rollouts_debug_stats", "obca_rollouts_debug_harness",
           "obca_rollouts_reset", "obca_rollouts_step", "obca_rollouts_read", "obca_rollouts_run",
           "obca_rollouts_set_mode", "obca_rollouts_queue_mode", "obca_set_shape_specialisation", "obca_shape_is_specialised", "obca_astar_batch", "obca_astar_workspace_bytes", "obca_primal_size", "obca_set_warm_start",
           "obca_rollouts_set_warm_start", "obca_dual_size", "obca_set_certificate_buffers", "obca_rasterise_batch",
           "obca_plan_clearance", "obca_plan_sweep", "obca_plan_tighten", "obca_rollouts_audit", "obca_rollouts_set_collision_stop", "obca_rollouts_set_exact_sensing",
           "obca_rollouts_read_clearance", "obca_rollouts_set_swept_rows", "obca_moving_rows_batch", "obca_plan_refine",
           "obca_grid_dilate_batch", "obca_route_resample", "obca_scene_select", "obca_grid_pool", "obca_pool_loop_init", "obca_pool_loop_advance",
           "obca_fleet_init", "obca_fleet_step", "obca_fleet_tracks_init", "obca_fleet_tracks", "obca_scene_select_staged",
           "obca_pool_tracks_init", "obca_pool_tracks", "obca_plan_tracks_init", "obca_plan_tracks")

OBCA_MAX_DYN = 4
RUN, DONE_GOAL, DONE_CAP, DONE_FAILED, DONE_COLLISION = 0, 1, 2, 3, 4
FLAG_NAMES = {RUN: "run", DONE_GOAL: "goal", DONE_CAP: "cap", DONE_FAILED: "failed", DONE_COLLISION: "collision"}
STATUS_SKIPPED = -5
STATUS_BAD_VARIANT = -6

STATUS_OK, STATUS_ACCEPTABLE, STATUS_INFEASIBLE = 0, 1, 2
STATUS_MAXITER, STATUS_LINESEARCH, STATUS_NUMERIC, STATUS_BAD_BOUNDS = -1, -2, -3, -4

_lib = None


def _bind_hip_runtime():
    """libobca_mpc.so names no HIP runtime of its own (no DT_NEEDED entry, see __graft_entry__.build): its hip* symbols
    bind to the runtime the process already uses, so device memory handed over by the host and our launches always live
    in ONE runtime, whatever the import order.  Under PyTorch-ROCm that is the copy torch ships (torch/lib/libamdhip64.so,
    loaded RTLD_LOCAL by torch -- re-opening the same file RTLD_GLOBAL only widens its visibility); without torch, the
    system runtime.  A C host that links libamdhip64 itself needs nothing of this."""
    cands = []
    try:
        import torch
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except ImportError:
        pass
    cands += ["libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"]
    err = None
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            return ctypes.CDLL(c, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            err = e
    raise RuntimeError("no HIP runtime (libamdhip64) could be loaded: %s" % err)


def load():
    """Load the shared library (built by __graft_entry__.build()); raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libobca_mpc.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(expected at %s). There is no CPU fallback." % LIB_PATH)
    _bind_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32p = ctypes.c_void_p, ctypes.c_void_p
    lib.obca_create.argtypes = [ctypes.POINTER(ObcaDims), ctypes.POINTER(ctypes.c_void_p)]
    lib.obca_create.restype = ctypes.c_int
    lib.obca_destroy.argtypes = [ctypes.c_void_p]
    lib.obca_destroy.restype = None
    lib.obca_solve_batch.argtypes = [ctypes.c_void_p, i32p, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp,
                                     ctypes.POINTER(ObcaParams), vp, vp, vp, i32p, i32p, vp, vp]
    lib.obca_solve_batch.restype = ctypes.c_int
    lib.obca_set_profile_buffer.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.obca_set_profile_buffer.restype = None
    lib.obca_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.obca_set_mode.restype = ctypes.c_int
    lib.obca_set_two_sided_sweep.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.obca_set_two_sided_sweep.restype = ctypes.c_int
    lib.obca_rollouts_create.argtypes = [ctypes.POINTER(ObcaRolloutDims), ctypes.POINTER(ctypes.c_void_p)]
    lib.obca_rollouts_create.restype = ctypes.c_int
    lib.obca_rollouts_destroy.argtypes = [ctypes.c_void_p]
    lib.obca_rollouts_destroy.restype = None
    lib.obca_rollouts_reset.argtypes = [ctypes.c_void_p, vp, vp, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double,
                                        ctypes.POINTER(ObcaParams), vp]
    lib.obca_rollouts_reset.restype = ctypes.c_int
    lib.obca_rollouts_step.argtypes = [ctypes.c_void_p, vp]
    lib.obca_rollouts_step.restype = ctypes.c_int
    lib.obca_rollouts_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, vp]
    lib.obca_rollouts_run.restype = ctypes.c_int
    lib.obca_rollouts_debug_harness.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, vp, ctypes.c_int32, vp, vp, vp, vp]
    lib.obca_rollouts_debug_harness.restype = ctypes.c_int
    lib.obca_rollouts_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.obca_rollouts_set_mode.restype = ctypes.c_int
    lib.obca_set_shape_specialisation.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.obca_set_shape_specialisation.restype = ctypes.c_int
    lib.obca_shape_is_specialised.argtypes = [ctypes.c_void_p]
    lib.obca_shape_is_specialised.restype = ctypes.c_int
    lib.obca_rollouts_queue_mode.argtypes = [ctypes.c_void_p]
    lib.obca_rollouts_queue_mode.restype = ctypes.c_int
    lib.obca_astar_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    lib.obca_astar_workspace_bytes.restype = ctypes.c_int64
    lib.obca_astar_batch.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp,
                                     ctypes.POINTER(ctypes.c_double), ctypes.c_int32, vp, vp, vp, ctypes.c_int64, vp]
    lib.obca_astar_batch.restype = ctypes.c_int
    lib.obca_rasterise_batch.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, vp, vp]
    lib.obca_rasterise_batch.restype = ctypes.c_int
    lib.obca_primal_size.argtypes = [ctypes.POINTER(ObcaDims)]
    lib.obca_primal_size.restype = ctypes.c_int64
    lib.obca_set_warm_start.argtypes = [ctypes.c_void_p, vp, vp, ctypes.c_double]
    lib.obca_set_warm_start.restype = ctypes.c_int
    lib.obca_dual_size.argtypes = [ctypes.POINTER(ObcaDims)]
    lib.obca_dual_size.restype = ctypes.c_int64
    lib.obca_set_certificate_buffers.argtypes = [ctypes.c_void_p, vp, vp]
    lib.obca_set_certificate_buffers.restype = ctypes.c_int
    lib.obca_rollouts_set_warm_start.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    lib.obca_rollouts_set_warm_start.restype = ctypes.c_int
    lib.obca_rollouts_read.argtypes = [ctypes.c_void_p] + [vp] * 11
    lib.obca_rollouts_read.restype = ctypes.c_int
    # the plan calls take one batch: ego, n_obs, m, N, B, variant, (tighten: status,) x, A, b ... device, stream
    plan_head = [ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, i32p]
    plan_xAb, plan_tail = [vp, vp, vp], [ctypes.c_int32, vp]
    lib.obca_plan_clearance.argtypes = plan_head + plan_xAb + [vp, i32p, i32p, vp] + plan_tail
    lib.obca_plan_clearance.restype = ctypes.c_int
    lib.obca_plan_sweep.argtypes = plan_head + plan_xAb + [ctypes.c_int32, vp, vp, i32p, i32p, i32p, vp] + plan_tail
    lib.obca_plan_sweep.restype = ctypes.c_int
    lib.obca_plan_tighten.argtypes = plan_head + [i32p] + plan_xAb + [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                                                      ctypes.c_double, vp, vp, i32p, vp] + plan_tail
    lib.obca_plan_tighten.restype = ctypes.c_int
    lib.obca_rollouts_audit.argtypes = [ctypes.c_void_p, ctypes.c_int32, vp, vp, i32p, i32p, i32p, i32p, vp, vp]
    lib.obca_rollouts_audit.restype = ctypes.c_int
    lib.obca_rollouts_set_collision_stop.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32]
    lib.obca_rollouts_set_collision_stop.restype = ctypes.c_int
    lib.obca_rollouts_set_exact_sensing.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.obca_rollouts_set_exact_sensing.restype = ctypes.c_int
    lib.obca_rollouts_read_clearance.argtypes = [ctypes.c_void_p, vp, vp]
    lib.obca_rollouts_read_clearance.restype = ctypes.c_int
    lib.obca_rollouts_set_swept_rows.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    lib.obca_rollouts_set_swept_rows.restype = ctypes.c_int
    lib.obca_moving_rows_batch.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp,
                                           ctypes.c_double, ctypes.c_double, vp, vp, ctypes.c_int32, vp]
    lib.obca_moving_rows_batch.restype = ctypes.c_int
    lib.obca_plan_refine.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, vp, i32p, ctypes.c_int32, vp, vp, i32p,
                                     ctypes.c_int32, vp]
    lib.obca_plan_refine.restype = ctypes.c_int
    lib.obca_grid_dilate_batch.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int32, vp]
    lib.obca_grid_dilate_batch.restype = ctypes.c_int
    lib.obca_route_resample.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, i32p, vp, vp, vp, i32p, ctypes.c_int32, vp]
    lib.obca_route_resample.restype = ctypes.c_int
    lib.obca_scene_select.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.c_int32] * 7 + [vp, vp, vp, vp, vp, vp, i32p, i32p, vp, i32p,
                                                                                                 vp, vp, i32p, i32p, vp, ctypes.c_int32, vp]
    lib.obca_scene_select.restype = ctypes.c_int
    lib.obca_grid_pool.argtypes = [vp] + [ctypes.c_int32] * 4 + [ctypes.c_double] * 3 + [vp, vp, i32p, i32p, i32p, ctypes.c_int32, vp]
    lib.obca_grid_pool.restype = ctypes.c_int
    lib.obca_pool_loop_init.argtypes = [ctypes.POINTER(ObcaPoolLoop)]
    lib.obca_pool_loop_init.restype = None
    lib.obca_pool_loop_advance.argtypes = [ctypes.POINTER(ObcaPoolLoop), ctypes.c_int32, ctypes.c_int32, vp]
    lib.obca_pool_loop_advance.restype = ctypes.c_int
    lib.obca_fleet_init.argtypes = [ctypes.POINTER(ObcaFleet)]
    lib.obca_fleet_init.restype = None
    lib.obca_fleet_step.argtypes = [ctypes.POINTER(ObcaFleet), ctypes.c_int32, ctypes.c_int32, vp]
    lib.obca_fleet_step.restype = ctypes.c_int
    lib.obca_fleet_tracks_init.argtypes = [ctypes.POINTER(ObcaFleetTracks)]
    lib.obca_fleet_tracks_init.restype = None
    lib.obca_fleet_tracks.argtypes = [ctypes.POINTER(ObcaFleetTracks), ctypes.c_int32, vp]
    lib.obca_fleet_tracks.restype = ctypes.c_int
    lib.obca_scene_select_staged.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.c_int32] * 7 + \
        [vp, vp, vp, vp, vp, vp, i32p, i32p, ctypes.c_int32, ctypes.c_int32, vp, vp, i32p, vp, i32p, vp, vp, i32p, i32p, vp,
         ctypes.c_int32, vp]
    lib.obca_scene_select_staged.restype = ctypes.c_int
    lib.obca_pool_tracks_init.argtypes = [ctypes.POINTER(ObcaPoolTracks)]
    lib.obca_pool_tracks_init.restype = None
    lib.obca_pool_tracks.argtypes = [ctypes.POINTER(ObcaPoolTracks), ctypes.c_int32, ctypes.c_int32, vp]
    lib.obca_pool_tracks.restype = ctypes.c_int
    lib.obca_plan_tracks_init.argtypes = [ctypes.POINTER(ObcaPlanTracks)]
    lib.obca_plan_tracks_init.restype = None
    lib.obca_plan_tracks.argtypes = [ctypes.POINTER(ObcaPlanTracks), ctypes.c_int32, vp]
    lib.obca_plan_tracks.restype = ctypes.c_int
    # test hook of csrc/obca_math_probe.hip (not in include/obca_mpc.h, not in EXPORTS): math_probe() below.  A library of an
    # older tree loaded beside this one for an A/B (OBCA_LIB, tools/ab_run.sh) has none; math_probe() on it raises.
    if hasattr(lib, "obca_math_probe"):
        lib.obca_math_probe.argtypes = [ctypes.c_int32, ctypes.c_int64, vp, vp, ctypes.c_int32, vp]
        lib.obca_math_probe.restype = ctypes.c_int
    lib.obca_lds_bytes.argtypes = [ctypes.POINTER(ObcaDims)]
    lib.obca_lds_bytes.restype = ctypes.c_int64
    lib.obca_strerror.argtypes = [ctypes.c_int]
    lib.obca_strerror.restype = ctypes.c_char_p
    lib.obca_params_init.argtypes = [ctypes.POINTER(ObcaParams)]
    lib.obca_params_init.restype = None
    lib.obca_version.argtypes = []
    lib.obca_version.restype = ctypes.c_char_p
    _lib = lib
    return lib


def ptr(t):
    """the address of tensor ``t`` as a C argument: NULL for None and for a tensor without elements (whose data_ptr() is 0)"""
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def stream_ptr(dev):
    """the current stream of torch device ``dev`` as a C argument"""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def device_index(dev):
    """the ordinal of torch device ``dev``; the current device's for a bare "cuda\""""
    import torch
    return dev.index if dev.index is not None else torch.cuda.current_device()


def check(code):
    if code != 0:
        raise RuntimeError("libobca_mpc: %s (code %d)" % (load().obca_strerror(code).decode(), code))


def launch(fn, *args, dev):
    """the call ``fn(*args, device, stream)`` on torch device ``dev`` and its current stream; raises on an error code"""
    check(fn(*args, device_index(dev), stream_ptr(dev)))


MATH_PROBE_KINDS = {"obca_log": 0, "log": 1, "obca_sincos": 2, "sin_cos": 3}


def math_probe(kind, x):
    """tests only: the device's elementary functions on the float64 CUDA tensor ``x`` (csrc/obca_math_probe.hip).  ``kind``:
    "obca_log" (csrc/obca_math.h) and "log" (device library) return a tensor like ``x``; "obca_sincos" (the shared reduction the
    solver calls) and "sin_cos" (separate library calls) return [n, 2]: sine, cosine"""
    import torch
    require_gpu("math_probe")
    assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.dim() == 1 and x.numel() > 0
    k = MATH_PROBE_KINDS[kind]
    out = torch.empty((x.numel(), 2) if k >= 2 else (x.numel(),), dtype=torch.float64, device=x.device)
    launch(load().obca_math_probe, k, x.numel(), ptr(x), ptr(out), dev=x.device)
    keep_alive(out, (x,), x.device)
    return out


def keep_alive(anchor, tensors, dev):
    """a launch is asynchronous: the tensors it reads must outlive it.  They are tied to ``anchor`` (the result: a second call
    before the stream drains must not free the first call's inputs) and recorded on the current stream of ``dev`` (the caching
    allocator keeps a freed block out of other streams' hands until this stream has passed the free point).  None is skipped."""
    import torch
    anchor._obca_keep = tuple(tensors)
    s = torch.cuda.current_stream(dev)
    for t in anchor._obca_keep:
        if t is not None:
            t.record_stream(s)


def require_gpu(who):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("%s needs a ROCm GPU; there is no CPU fallback on the product path" % who)
