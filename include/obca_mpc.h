/*
 * obca_mpc.h -- C ABI of the MI355X batched OBCA-MPC solver (libobca_mpc.so).
 *
 * Drop-in boundary.  The reference has no FFI: the hot path is entered through plain Python method
 * calls on `obca()` (reference src/closed_loop.py:22, call sites :117-120, :130-140, :381-398).  Each
 * entry point below therefore names the reference interface it stands behind:
 *
 *   obca_create / obca_destroy   construction of the solver object   (src/closed_loop.py:22  `obca()`)
 *   obca_solve_batch             obca.obca_mpc4 / obca_mpc6 / obca_mpc8 (src/obca.py:828, :1361, :1564),
 *                                B independent calls at once
 *   obca_strerror                the reference never raises across this boundary (bare `except:`,
 *                                src/obca.py:1062-1065); errors are return codes / per-instance status
 *
 * All array arguments are DEVICE pointers (HBM resident, e.g. torch `data_ptr()`), row-major, fp64
 * unless noted; the caller owns every buffer.  Calls are asynchronous on the given HIP stream.
 * No C++ exception crosses this boundary.
 *
 * Threading: handles are independent; calls on ONE handle must be issued from one thread at a time and, when the
 * lane-per-instance kernel runs (it owns a workspace inside the handle), must be ordered on one stream.  Different
 * handles may be used concurrently from different threads and streams.
 */
#ifndef OBCA_MPC_H
#define OBCA_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_MAX_OBST 8      /* obstacles per instance                               */
#define OBCA_MAX_EDGES 4     /* half-spaces per obstacle (vObs[i]-1 in the reference) */

/* problem shape shared by every instance of a handle (reference arguments N, nObs, vObs) */
typedef struct obca_dims {
    int32_t N;                         /* horizon (reference argument N)                          */
    int32_t n_obs;                     /* obstacles passed to the solver (reference nObs)         */
    int32_t m[OBCA_MAX_OBST];          /* half-spaces of obstacle i = vObs[i]-1                   */
    int32_t max_batch;                 /* largest B later passed to obca_solve_batch              */
    int32_t device;                    /* HIP device ordinal                                      */
} obca_dims;

/* cost weights of one call family (reference arguments P, Q, R=[R1,R2]) */
typedef struct obca_weights {
    double Q[9], P[9], R1[4], R2[4];
} obca_weights;

/* everything else the reference passes per call and keeps constant over a rollout */
typedef struct obca_params {
    uint32_t struct_size;              /* sizeof(obca_params) of the header the CALLER was built against: set by
                                          obca_params_init() (or by hand after zero-initialising).  Anything else -- a caller built
                                          against another layout, a struct that was never initialised -- is answered with
                                          OBCA_E_INVAL instead of being read field by field as something it is not          */
    uint32_t time_bound;               /* [OBCA_TIME_BOUND_REFERENCE] one of the OBCA_TIME_BOUND_* constants below: how variant 4
                                          bounds its time scale (the word that was `reserved_`, documented as 0, until obca_mpc 0.16:
                                          size and every offset are unchanged, and the zeroed struct of an older caller means the
                                          reference's bound); anything else: OBCA_E_INVAL             */
    obca_weights free_time;            /* used by variant 4 (closed_loop.py:77-81)                */
    obca_weights fixed_time;           /* used by variants 6 and 8 (closed_loop.py:94-98)         */
    double xL[2], xU[2];               /* position box (theta is unbounded, obca.py:916)          */
    double uL[2], uU[2];               /* input box                                               */
    double ego[4];                     /* car footprint (closed_loop.py:63)                       */
    double dmin;                       /* clearance (closed_loop.py:64)                           */
    /* interior-point options; <= 0 selects the default in brackets.  The struct MUST be zero-initialised before its fields
       are set (memset / = {0}): every option added later reads 0 as "default". */
    double tol;                        /* [1e-8]  IPOPT tol                                        */
    double rho;                        /* [1e4]   elastic (l1) penalty, unscaled objective units; a free-time solve
                                                   that ends with elastic variables left is repeated from the same
                                                   start with rho x 100 and, if they still remain, with rho x 1000
                                                   (exact-penalty escalation; the next start begins at rho again)  */
    double feas_tol;                   /* [1e-6]  largest elastic variable still called feasible   */
    int32_t max_iter_free;             /* [3000]  IPOPT default, variant 4: bounds EACH pass of a solve (see `patience`) */
    int32_t max_iter_fixed;            /* [1000]  obca.py:1538, variants 6/8: likewise              */
    int32_t max_soc;                   /* [4]     IPOPT max_soc: second-order-correction trials after a rejected first
                                                   trial step; 0 = the default, negative = off              */
    /* The starts of a solve ("start ladder"; rule and measurements: oracle/ipm_dense.py:solve).  A solve
       that ends without a feasible point -- status 2, -1, -2, -3 -- is repeated from the next start of the order, inside the
       same launch, until one start ends feasible or the order is exhausted; iteration and factorisation counts returned are
       those of the whole sequence; status, iterate and info[0..2] are those of the pass that ended feasible.  After an exhausted
       ladder (obca_mpc 0.6; before: the last pass's, whatever it was) they are those of the most informative pass: the FIRST
       one, replaced by a later one only if that one converged to a stationary point of the penalty problem with elastic
       variables left (status 2 -- a statement about the problem) where the held one did not (-1, -2, -3 -- statements about the
       solver), or if it is the same start's repetition with a raised penalty.  So status 2 after an exhausted ladder means
       "some start converged and found no feasible point", -1 / -2 / -3 that none converged.  The three starts:
         x0      every variable 0, Topt = 1 as the reference (src/obca.py:856), every pose at x0 -- the iterate IPOPT's first
                 Newton step reaches from the reference's all-zero start (the initial condition and the dynamics linearised
                 at v = 0 read x_k = x0); uses nothing but x0, like the reference's cold start
         window  the poses of the reference window xref (first pose x0), inputs by differences clipped to their box
         zeros   the reference's literal start: every variable 0, Topt = 1
       No order makes a problem infeasible that another order solves: all three starts are tried in every order. */
    int32_t start_order;               /* [OBCA_START_DEFAULT] one of the OBCA_START_* constants below; anything else:
                                                   OBCA_E_INVAL                                             */
    int32_t single_start;              /* [0]     1 = only the first start of the order (with its penalty escalation) -- what a
                                                   driver asks for where its own fallback follows, as obca_mpc8 follows a
                                                   failed obca_mpc6 in the closed loop (src/closed_loop.py:393-398);
                                                   other values than 0 / 1: OBCA_E_INVAL                    */
    int32_t patience;                  /* [500 + 10 N]  while further starts remain, the FIRST start's passes are abandoned
                                                   for the next start after this many iterations (solves converge far below
                                                   it or crawl until max_iter); never above max_iter_*; with
                                                   single_start = 1 only max_iter_* applies                 */
    int32_t retry_iter;                /* [300 + 10 N]  iteration limit of every later start's passes; never above max_iter_* */
    int32_t dodge;                     /* [on]    0 = the default (on), negative = off.  The last rung of the ladder, obca_mpc6 /
                                                   obca_mpc8 only, after every start of the order (the one start with
                                                   single_start = 1) ended without a feasible point: where the reference window
                                                   runs head-on into an obstacle the penalty problem has a stationary point that is
                                                   symmetric about the window (the plan brakes in front of the obstacle) and all
                                                   three starts end there although a plan around the obstacle exists -- steps 21-25
                                                   of the reference's own demo11 run, where IPOPT drives around.  Two more passes
                                                   start from the window moved 3 m to the right and to the left of the direction of
                                                   travel (ramped in over three stages; lambda, mu on the separating half-space);
                                                   both run, the feasible answer with the lower objective is returned; their
                                                   iterations are added to `iters`.  obca_mpc8 only (obca_mpc 0.6; its failure has no
                                                   fallback behind it): if neither side ends feasible, the same two starts once more
                                                   with IPOPT's own mu_init 0.1 instead of 1 (csrc/obca_device.h: OBCA_DODGE_LEVEL2_MU).  A failed rung leaves the answer the order's
                                                   starts left (see above).                                    */
    int32_t terminal_screen;           /* [on]    0 = the default (on), negative = off.  obca_mpc6 whose terminal set
                                                   x_N >= term[0] no trajectory can reach -- the first step's heading is x0's, the
                                                   speeds are bounded by uL / uU and, from u0, by the acceleration rows; margin for
                                                   elastic variables of size feas_tol on the rows involved -- is not run: status
                                                   OBCA_STATUS_INFEASIBLE, iters 0, xopt = x0 at every stage, uopt = 0,
                                                   info = (0, shortfall in metres, 0, 0).  The reference's closed loop asks for
                                                   x0 + 5 m in N_fix steps of exactly 1 m at full speed, so after the first dodge
                                                   four of five failing obca_mpc6 calls are of this kind (tests/test_terminal_screen.py) */
} obca_params;

/* zero-fills *p and sets struct_size: the one way to start filling an obca_params */
void obca_params_init(obca_params* p);

/* obca_params.start_order */
enum {
    OBCA_START_DEFAULT = 0,            /* window -> x0 -> zeros for every variant.  obca_mpc6 / obca_mpc8 have several local optima, and from the
                                          window the solver ends at the lower one far more often; obca_mpc4 has one optimum on every workload
                                          measured -- all 8192 headline instances, the free-time half of config C3, every free-time step of the
                                          five reference-held runs end where they end from x0 -- and reaches it from the window in a third of the
                                          iterations (csrc/obca_device.h: OBCA_EFFECTIVE_ORDER; x0 first was the obca_mpc4 default of obca_mpc 0.4).
                                          Two exceptions keep x0 first for every variant: single_start = 1 (a caller with its own fallback wants the
                                          start that fails fastest: the closed loop's obca_mpc6 before obca_mpc8) and obca_set_warm_start (the stored
                                          plan stands for x0).  A caller whose reference window is no trajectory (start and goal only: the open-loop
                                          plan) is served better by OBCA_START_X0_FIRST: the x0 start then also runs under `patience` instead of the smaller
                                          `retry_iter` (demo9 at N >= 66 needs 600-1300 iterations from x0) -- the Python mirror's open-loop plan passes it
                                          per call (closedLoop.mpc_openLoop_freeTime). */
    OBCA_START_WINDOW_FIRST = 1,       /* window -> x0 -> zeros, also for single-start and warm-started calls */
    OBCA_START_ZEROS_FIRST = 2,        /* zeros -> window -> x0: the reference's literal start first (the default of
                                          obca_mpc 0.1)                                            */
    OBCA_START_X0_FIRST = 3            /* x0 -> window -> zeros for every variant (the default of obca_mpc 0.2 / 0.3; obca_mpc4's until 0.4) */
};

/* obca_params.time_bound: the upper bound Tmax of obca_mpc4's time scale T (the step length is T * Ts; OBCA_T_MIN <= T <= Tmax),
   Tmax = dis / (N * uU[0] * Ts) + 1 with `dis` the distance the window asks the car to cover.  Only variant 4 reads it: the
   fixed-time variants have no time scale. */
enum {
    OBCA_TIME_BOUND_REFERENCE = 0,     /* the reference's: dis = (xref_N.x - x0.x) + (xref_N.y - x0.y), a SIGNED sum (src/obca.py;
                                          SURVEY.md quirk q3).  A window that runs towards smaller x or smaller y gets a bound
                                          below what the car needs -- below 1, even below OBCA_T_MIN -- and the problem is
                                          infeasible by construction.  The default: every output word is the one obca_mpc 0.16
                                          returned. */
    OBCA_TIME_BOUND_PATH = 1           /* dis = sum_{k=1..N} (|px_k - px_{k-1}| + |py_k - py_{k-1}|), p_0 = x0[:2], p_k = xref[:2,k]:
                                          the L1 arc length of the window, summed in the order k = 1 .. N from 0.0, each term
                                          (|dx| + |dy|) formed first.  The arc length and not the distance of the end points: a
                                          window round a box turns back, and the end points understate the route.  L1 and not
                                          Euclidean: it is the reference's own formula read without a direction -- the same word
                                          wherever the window is monotone in x and in y and the sums are exact, never below the
                                          reference's value up to rounding, and Tmax never below 1. */
};


typedef struct obca_handle obca_handle;

/* per-instance status written by obca_solve_batch */
enum {
    OBCA_STATUS_OK = 0,                /* converged to tol                                        */
    OBCA_STATUS_ACCEPTABLE = 1,        /* IPOPT "acceptable" termination                          */
    OBCA_STATUS_INFEASIBLE = 2,        /* converged but elastic variables remain (feas = False)   */
    OBCA_STATUS_MAXITER = -1,
    OBCA_STATUS_LINESEARCH = -2,
    OBCA_STATUS_NUMERIC = -3,
    OBCA_STATUS_BAD_BOUNDS = -4,
    OBCA_STATUS_SKIPPED = -5,          /* variant[b] == 0: instance not solved, outputs untouched */
    OBCA_STATUS_BAD_VARIANT = -6       /* variant[b] not in {0,4,6,8}, or 6 with term == NULL: not solved */
};

/* return codes */
enum {
    OBCA_OK = 0,
    OBCA_E_INVAL = -22,                /* bad argument / shape beyond compiled limits             */
    OBCA_E_NOMEM = -12,
    OBCA_E_HIP = -5,                   /* a HIP runtime call failed                               */
    OBCA_E_LDS = -28                   /* shape does not fit the LDS kernel (mode 1 only)         */
};

int obca_create(const obca_dims* dims, obca_handle** out);
void obca_destroy(obca_handle* h);

/*
 * Solve B independent NLPs.  variant[b] in {4, 6, 8} selects obca_mpc4 / obca_mpc6 / obca_mpc8;
 * variant[b] == 0 skips instance b (status OBCA_STATUS_SKIPPED, outputs untouched) so that a device-side
 * driver can mask instances without a host round trip.
 *   x0    [B,3]          current pose                     (reference x0)
 *   u0    [B,2]          previous input                   (reference u0)
 *   xref  [B,3,N+1]      reference window                 (reference xref[:, :N+1])
 *   A     [B,N+1,M,2]    obstacle rows per horizon step   (reference AObs; variant 4 reads step 0 only,
 *   b     [B,N+1,M]       obca.py:969; M = sum m[i])      (reference bObs)
 *   Ts    [B]            base sample time                 (reference Ts)
 *   term  [B,3]          xmin, ymin, ymax of the terminal set, variant 6 only (obca.py:1465-1466); may be NULL when
 *                        no instance is variant 6 (a variant-6 instance then gets OBCA_STATUS_BAD_VARIANT)
 * outputs
 *   xopt  [B,3,N+1], uopt [B,2,N], ts_opt [B] (= Topt*Ts for variant 4, Ts otherwise)
 *   status [B] int32, iters [B] int32
 *   info  [B,4] or NULL: objective value, largest elastic variable, final optimality error,
 *                        number of KKT factorisations
 */
int obca_solve_batch(obca_handle* h, const int32_t* variant, int32_t B,
                     const double* x0, const double* u0, const double* xref,
                     const double* A, const double* b, const double* Ts, const double* term,
                     const obca_params* params,
                     double* xopt, double* uopt, double* ts_opt, int32_t* status, int32_t* iters,
                     double* info, void* hip_stream);

/* Optional warm start -- NOT reference behaviour (every solve of the reference is a cold start from zeros, T = 1,
 * src/obca.py:856), off by default, for receding-horizon callers that re-solve a problem one step later.
 * z: device buffer [max_batch, obca_primal_size(dims)] owned by the caller.  While set, every solve that ends
 * converged/acceptable stores its primal vector (poses, inputs, lambda, mu, time scale) there, and every solve of an
 * instance b with use[b] != 0 (use == NULL: all) starts from the stored vector moved one horizon stage forward (last
 * stage repeated) with barrier parameter mu_init instead of 0.1.  Which local optimum is found may differ from the cold
 * start's.  z == NULL switches it off. */
int64_t obca_primal_size(const obca_dims* dims);
int obca_set_warm_start(obca_handle* h, double* z, const int32_t* use, double mu_init);

/* Optional certificate output -- NOT part of the reference's call surface (its callers only read sol.value(x), sol.value(u),
 * src/obca.py:1057-1059), for KKT certificates of the ORIGINAL NLP at the returned point.  While set, every solve stores
 *   z [max_batch, obca_primal_size(dims)]  its final primal vector: per stage k the pose (3), the input (2, k < N),
 *                                          lambda_k (M) and mu_k (4 n_obs); the time scale Topt last (variant 4)
 *   y [max_batch, obca_dual_size(dims)]    the multipliers of the NLP's constraint rows in the objective's own units
 *                                          (the solver's internal objective scaling undone), sign convention
 *                                          grad f + sum_r y_r grad g_r = 0, rows in the order
 *                                            x_0 == x0 (3), dynamics (3N), [x_N == xref_N (3): variant 4],
 *                                            position box (2(N+1)), input box (2N), acceleration rows (2N),
 *                                            [Topt > 0, Topt bounds (2; each stands for the N+1 tied copies): variant 4],
 *                                            [terminal set x, y (2): variant 6], ||A'lambda||^2 <= 1 (per stage and obstacle),
 *                                            distance rows (per stage and obstacle), lambda >= 0 ((N+1) M), mu >= 0 ((N+1) 4 n_obs),
 *                                          followed by the rotation equalities (2 per stage and obstacle).
 * Either pointer may be NULL; both NULL switches it off. */
int64_t obca_dual_size(const obca_dims* dims);
int obca_set_certificate_buffers(obca_handle* h, double* z, double* y);

/* Kernel selection: 0 = auto (default; also env OBCA_MODE): one wavefront per instance when its rows fit the
 * wavefront's registers (<= 384 rows) and its working set one CU's LDS; beyond that, shapes with at most three obstacles run one
 * wavefront per instance with the row state in an HBM workspace owned by the handle (measured 6-33 % faster than four wavefronts
 * there: the stage-serial sweep dominates and four times as many instances are in flight), shapes with more obstacles four
 * wavefronts per instance while the working set still fits the LDS (<= 1280 rows, e.g. N = 20 with five obstacles); else four
 * wavefronts per instance with the row state and every O(rows) array in the HBM workspace and only the O(N) blocks of the
 * stage-serial Riccati sweep in LDS (long horizons: N = 74 with five obstacles has 3976 rows; every shape obca_create accepts,
 * N <= 127, fits there); the lane-per-instance kernel only where the runtime refuses those kernels their LDS.  The choice is a
 * function of the shape and the mode, never of the batch size -- and, once the handle's HBM workspace could not be allocated,
 * of that fact: auto mode then stays with the LDS-resident kernels where they hold the shape (csrc/obca_select.h: plan).
 * 1 = one wavefront per instance; 2 = lane-per-instance (64 instances per wavefront, working set in an HBM workspace
 * owned by the handle; any shape); 3 = four wavefronts per instance, LDS resident; 4 = four wavefronts per instance, HBM
 * workspace; 5 = one wavefront per instance, HBM workspace.  Returns OBCA_E_LDS if mode 1 / 3 / 4 / 5 cannot hold the shape. */
int obca_set_mode(obca_handle* h, int mode);

/* Compile-time-shape instantiations.  For the problem shapes the reference's closed-loop driver produces with its nine demo
 * settings (N = 5 or 6; static obstacles plus sensed moving rectangles: (obstacles, rows) = (2, 2) (3, 6) (4, 10) (5, 14) (6, 18))
 * and for the two halves of the N = 20 benchmark configuration (list: csrc/obca_device.h OBCA_SHAPES, OBCA_MW_SHAPES) the library
 * holds an instantiation of the kernel with the shape as compile-time constants -- same code, same arithmetic, every output word
 * equal (tests/test_gpu_shapes.py), 5-15 % shorter launches.  obca_solve_batch uses it whenever the handle's shape is one of them
 * and the kernel selection above would run the corresponding generic kernel; on = 0
 * (environment at obca_create: OBCA_SPECIALISE=0) forces the generic kernel.  obca_shape_is_specialised: 1 if launches of this
 * handle use an instantiation. */
int obca_set_shape_specialisation(obca_handle* h, int on);
int obca_shape_is_specialised(const obca_handle* h);

/* Four-wavefront kernels (OBCA_MODE 3, and auto mode for shapes whose rows do not fit one wavefront's registers): the
 * Riccati sweep over the stages can be cut at stage ~0.45 N into a backward half (cost-to-go) and a forward half
 * (cost-to-arrive) that two wavefronts run at the same time, meeting in one 6 x 6 solve.  Same Newton step up to
 * roundoff (measured in the kernel: 1e-11..1e-10 of the step's size typically); the one-sided sweep rounds exactly like
 * the one-wavefront kernels.  on = -1 (default): two-sided exactly where the one-wavefront kernels cannot run the
 * shape, so that every shape both kernel families can run gives bit-identical results in both; 0: never; 1: always.
 * Environment override at obca_create: OBCA_TWO_SIDED=-1|0|1. */
int obca_set_two_sided_sweep(obca_handle* h, int on);

/* Diagnostic: device buffer [max_batch,20] receiving per-phase shader-clock totals of each instance.
 * Only builds compiled with -DOBCA_PROFILE write to it; NULL (the default) disables it. */
void obca_set_profile_buffer(obca_handle* h, double* prof);

/* bytes of LDS one instance needs in the wave-per-instance kernels (> 163840: they cannot run it); the
 * four-wavefront kernels ask for 8 * (36 * ((N + 1) / 2) + 42) bytes more (forward half of their two-sided Riccati sweep),
 * beyond 768 rows another 8 * (15 * (max(rows - 1024, 0) + 1) + 1025) (fifth row slot and row values, csrc/obca_device.h).
 * A launch additionally asks for the scratch of the second-order correction (8 * even(variables + 2 rows + 2 (N + 1) n_obs)
 * bytes) where that lives in LDS: where it costs the one-wavefront kernels no occupancy, and where the four-wavefront
 * kernels' total stays within one CU's 160 KiB (csrc/obca_device.h: obca_soc_lds_wave / _mw). */
int64_t obca_lds_bytes(const obca_dims* dims);

/* ------------------------------------------------------------------------------------------------------
 * Device-resident closed loop: B receding-horizon rollouts advanced in lock-step without leaving the GPU.
 *
 * Stands behind the body of the reference's `closedLoop.closed_loop_mpc4` loop (src/closed_loop.py:345-432):
 * update_obstacle (:445-486), sensor (:591-629), update_reference_trajectory (:502-528), the fixed-time
 * reference preparation (:360-374 with update_path(allAviable=1) :570-587), rebuild_lObs + obstacle_H_Represent
 * for the moving rectangles (src/demo_setting.py:457-473, src/model_obstacle.py:37-102), the variant dispatch
 * with the mpc6 -> mpc8 fallback (:380-398) and the state advance (:400-432).  Quirks kept: q7 (Ts overwritten
 * after a fixed-time step), q8 (vertex lists of present obstacles are not filtered by the lidar gate), cold start
 * every solve, stop after max_steps (30) steps.  N_free = N, N_fix = N_fix (default: equal, the reference's 6/6).
 *
 * Static obstacles are passed as their half-space rows (host side: obstacle_H_Represent); moving obstacles as the
 * reference's 11-tuple [cx, cy, theta, length, width, speed, end_x, end_y, end_theta, t_start, t_end] followed by
 * cos(theta), sin(theta) as the host evaluated them (13 doubles), so that the exact `==` branch tests of
 * obstacle_H_Represent see the same numbers as the reference.
 */
#define OBCA_MAX_DYN 4

typedef struct obca_rollout_dims {
    int32_t N;                         /* horizon of both the free-time and the fixed-time problem */
    int32_t n_static;                  /* static obstacles                                          */
    int32_t m_static[OBCA_MAX_OBST];   /* their half-space counts                                   */
    int32_t n_dyn;                     /* moving rectangles per rollout, 0..OBCA_MAX_DYN             */
    int32_t path_max;                  /* padded length of the reference path                       */
    int32_t batch;                     /* rollouts                                                  */
    int32_t max_steps;                 /* 30 in the reference (src/closed_loop.py:431)              */
    int32_t device;
    int32_t N_fix;                     /* horizon of the fixed-time problem (reference N_fix); 0 = N.  Must be a multiple of
                                          N (the reference resamples the reference plan by int(N_fix/N_free),
                                          src/closed_loop.py:570-587) with N_fix - 5 <= N (its shift-in of the previous plan,
                                          :363-364, reads N_fix - 5 + 1 columns of a free-time plan; the reference raises
                                          IndexError beyond that, e.g. at 6/12)                       */
} obca_rollout_dims;

typedef struct obca_rollouts obca_rollouts;

/* rollout flags */
enum { OBCA_RUN = 0, OBCA_DONE_GOAL = 1, OBCA_DONE_CAP = 2, OBCA_DONE_FAILED = 3, OBCA_DONE_COLLISION = 4 };

int obca_rollouts_create(const obca_rollout_dims* dims, obca_rollouts** out);
void obca_rollouts_destroy(obca_rollouts* r);

/* (Re)start all rollouts.  Device pointers: start [B,3], goal [B,2], path [B,3,path_max] (A* reference,
 * row-major x/y/yaw), path_len [B] int32, static_A [B,Ms,2], static_b [B,Ms], dyn [B,n_dyn,13].
 * Ts0 = the reference's self.Ts (0.1), sense_dis = setting.senseDis (10). */
int obca_rollouts_reset(obca_rollouts* r, const double* start, const double* goal, const double* path,
                        const int32_t* path_len, const double* static_A, const double* static_b, const double* dyn,
                        double Ts0, double sense_dis, const obca_params* params, void* hip_stream);

/* One iteration of the loop body for every rollout still running: harness kernel, one solve launch per problem
 * shape (variant 4 on the static obstacles; variant 6, then 8 where 6 failed, per number of sensed obstacles),
 * state advance.  Asynchronous; no host synchronisation inside. */
int obca_rollouts_step(obca_rollouts* r, void* hip_stream);

/* n_steps iterations for every rollout.  Default (mode 0): when every problem shape fits the wave kernel, ONE launch
 * of a persistent kernel (harness on lane 0, solves on the wave) whose workgroups -- one per SIMD -- take (round, rollout)
 * items (a round = six consecutive steps) from a device-side queue: every rollout has done round r before any starts
 * round r + 1, rollouts advance independently instead of in lock step (one expensive solve does not hold the batch back),
 * and the launch does not end with a few long rollouts on an otherwise idle GPU.  There is one queue per XCD (rollout b
 * belongs to queue b % 8 and is only handled by workgroups running on that XCD, so its state is handed on inside the XCD's
 * L2 without a write-back), followed by one pass of a global queue that skips every item already done.  Results are
 * identical to n_steps calls of obca_rollouts_step.  OBCA_ROLLOUT_QUEUE at obca_rollouts_create: 2 (default) as described,
 * 1 the global queue only (hand-offs through HBM with agent-scope release / acquire), 0 one workgroup per rollout for all
 * its steps.  Mode 1 forces the lock-step launches. */
int obca_rollouts_run(obca_rollouts* r, int32_t n_steps, void* hip_stream);
int obca_rollouts_set_mode(obca_rollouts* r, int mode);
/* The queue mode obca_rollouts_run uses (2, 1 or 0 as above).  2 is only offered where the device reports eight XCCs
 * (hipDeviceAttributeNumberOfXccs; MI355X): the per-XCD queues identify an L2 by HW_REG_XCC_ID & 7.  Elsewhere the default is 1. */
int obca_rollouts_queue_mode(const obca_rollouts* r);
/* Diagnostic (-DOBCA_RO_STATS builds): per persistent workgroup [wait, work (10 ns units), items, end clock], n <= 16384 ints to host */
int obca_rollouts_debug_stats(obca_rollouts* r, int32_t* out, int n);
/* Test hook: runs ONLY the harness part of a step (obstacle advance, lidar gate, reference window, fixed-time preparation,
 * half-space rows of the moving rectangles -- everything before the solve) for every rollout, after setting its step counter
 * to k, its inherited step length to Ts_opt and (x0_host != NULL) its pose to x0_host[3]; then copies what the harness handed
 * the solver of group g (= number of sensed moving obstacles) to HOST buffers: variant [B] (0: the rollout is not in this
 * group), A [B,N_g+1,M_g,2], b [B,N_g+1,M_g] with M_g = static rows + 4 g, N_g = N (g = 0) or N_fix.  Synchronises.  The
 * rollout state is left as the harness left it (moving obstacles advanced): obca_rollouts_reset before running on. */
int obca_rollouts_debug_harness(obca_rollouts* r, int32_t k, double Ts_opt, const double* x0_host, int32_t g,
                                int32_t* variant, double* A, double* b, void* hip_stream);

/* Optional, NOT reference behaviour (see obca_set_warm_start): a step whose problem shape equals the previous step's
 * starts from the previous plan moved one stage forward with barrier parameter mu_init.  Call before
 * obca_rollouts_reset; enable = 0 restores the reference's cold starts. */
int obca_rollouts_set_warm_start(obca_rollouts* r, int enable, double mu_init);

/* Optional collision stop (obca_mpc 0.7), the simulator's contact check -- NOT what the controller knows: after every
 * applied step k, interval k (knot k -> k + 1) is measured exactly as obca_rollouts_audit measures it (static rows and
 * EVERY present moving box, sensed or not; n_sub + 1 samples).  Its smallest sample (certified = 1: the certified lower
 * bound) is recorded; below `clearance` (metres) the rollout ends with OBCA_DONE_COLLISION, which wins over GOAL / CAP
 * of the same step.  The colliding step stays in the history: a stopped rollout's history equals the unstopped one's
 * cut after steps = first collision + 1.  n_sub = 0: off (default); else 1..63.  clearance finite, certified 0 / 1;
 * anything else: OBCA_E_INVAL without side effect.  Call before obca_rollouts_reset, like obca_rollouts_set_warm_start. */
int obca_rollouts_set_collision_stop(obca_rollouts* r, int32_t n_sub, double clearance, int32_t certified);
/* Optional, NOT reference behaviour: on = 1 hands the solver the j-th SENSED box's own rectangle, moved with its own
 * velocity; on = 0 (default) keeps the reference's sensor pairing (the j-th PRESENT box's rectangle with the j-th sensed
 * box's velocity).  Same problem shapes either way.  on outside {0, 1}: OBCA_E_INVAL.  Call before obca_rollouts_reset. */
int obca_rollouts_set_exact_sensing(obca_rollouts* r, int32_t on);
/* Optional swept, inflated rows of the sensed moving boxes (obca_mpc 0.8), NOT reference behaviour: stage kk of a
 * fixed-time problem gets, for every sensed box, the four rows of the rectangle that covers the box -- inflated by `margin`
 * metres -- at every stage time in [kk - half_window, kk + half_window] (same heading, centre at the box's stage-kk
 * position, length + 2 (half_window |Ts_opt v| + margin), width + 2 margin) instead of the rows of the box at stage kk.
 * Same problem shapes, same kernels.  With half_window >= 1/2 a feasible obca_mpc6 / obca_mpc8 step keeps the interpolated
 * car at least dmin + margin - half_window delta - eps away from every box sensed at that step, delta = |dp| + r_max
 * |dtheta| of the applied interval (derivation, eps: csrc/obca_rollout_core.h, moving_box_rows); a grown box can swallow
 * the fixed stage-0 pose, which ends the rollout as OBCA_DONE_FAILED.  Both zero: off (default), every word as without
 * the call.  half_window in [0, 1], margin in [0, 2], finite; anything else: OBCA_E_INVAL without side effect.  Needs exact
 * sensing (the box's own rectangle AND velocity): obca_rollouts_reset returns OBCA_E_INVAL, before it touches anything,
 * while swept rows are on and exact sensing is off.  Call before obca_rollouts_reset.  obca_rollouts_debug_harness shows
 * the swept rows as the solver gets them. */
int obca_rollouts_set_swept_rows(obca_rollouts* r, double half_window, double margin);
/* Clearance history of the collision stop to a caller-owned DEVICE buffer clear_hist [B,max_steps]: the measured value
 * of every interval the stop evaluated, +inf elsewhere (stop off, or beyond the rollout's steps).  Asynchronous. */
int obca_rollouts_read_clearance(obca_rollouts* r, double* clear_hist, void* hip_stream);

/* Copy state and history to caller-owned DEVICE buffers (any may be NULL): x_closed [B,max_steps+1,3],
 * u_closed [B,max_steps,2], T_closed [B,max_steps], x_openloop [B,max_steps,3,max(N,N_fix)+1] (a free-time
 * plan fills its first N+1 columns), variant_hist [B,max_steps]
 * int32 (4/6/8 as solved, 0 = no step), iters_hist [B,max_steps] int32, status_hist [B,max_steps] int32 (solver
 * status of the step's last solve), dyn_hist [B,max_steps,n_dyn,4]
 * (cx, cy, present, sensed), steps [B] int32 (successful steps), flags [B] int32. */
int obca_rollouts_read(obca_rollouts* r, double* x_closed, double* u_closed, double* T_closed, double* x_openloop,
                       int32_t* variant_hist, int32_t* iters_hist, int32_t* status_hist, double* dyn_hist, int32_t* steps,
                       int32_t* flags, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Batched global planner: the reference's grid A* (src/a_star.py:16-102: 8-connected, Euclidean cost and
 * heuristic, open list ordered by (f, (row, col)), its neighbour order and re-queue rules) followed by
 * rebuild_path (:137-147) and create_reference_path (:189-200), one rollout per GPU lane.
 *   grid  [B,rows,cols] uint8, 1 = occupied (setting.org_gridMap);  start, goal [B,2] int32 as (row, col)
 *         = (pose_y, pose_x) like the reference's call (src/closed_loop.py:28-30);  rows*cols <= 65535
 *   yaw9  HOST pointer, 9 doubles: arctan2(dy, dx) for dy, dx in {-1,0,1} at index (dy+1)*3+(dx+1), as the
 *         caller's libm evaluates them (the reference uses numpy's)
 *   path  [B,3,path_max] x / y / yaw rows, padded with the last point; path_len [B]: points, or
 *         -1 no route (an occupied goal included; an occupied start is left like any other cell), -2 open list
 *         overflow, -3 path_max too small, -4 start or goal outside [0,rows) x [0,cols): that instance returns before
 *         it touches its workspace.  The path of an instance with a negative code is not written.
 *   workspace: device buffer of obca_astar_workspace_bytes(B, rows, cols) bytes.
 * path / path_len are what obca_rollouts_reset takes. */
int64_t obca_astar_workspace_bytes(int32_t B, int32_t rows, int32_t cols);
int obca_astar_batch(const uint8_t* grid, int32_t B, int32_t rows, int32_t cols, const int32_t* start,
                     const int32_t* goal, const double* yaw9, int32_t path_max, double* path, int32_t* path_len,
                     void* workspace, int64_t workspace_bytes, void* hip_stream);

/* Occupancy grids of B worlds on the device -- the reference's mapModel.shape2grid (src/model_map.py:21-56; vertex
 * re-ordering :88-101 and the division by the resolution :58-71 included): boxes [B,K,4] = (xmin, ymin, xmax, ymax) of each
 * obstacle polygon in world units (an entry with xmin > xmax or NaN is padding), grid [B,rows,cols] uint8 (1 = occupied),
 * rows = int((map_y - 1)/resolution) + 1, cols likewise (src/model_map.py:17).  Cells x .. x + int(xmax/res - xmin/res),
 * y .. y + int(ymax/res - ymin/res) are set, x = int(xmin/res), y = int(ymin/res) (truncation towards zero), CLIPPED to the
 * map: the part of a box outside the grid is dropped, a box wholly outside marks nothing (the reference raises there).  Box
 * coordinates divided by the resolution have to fit an int32.  The grid is what obca_astar_batch takes. */
int obca_rasterise_batch(const double* boxes, int32_t B, int32_t K, double resolution, int32_t rows, int32_t cols,
                         uint8_t* grid, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Collision audit: true clearance in fp64 between the car footprint (ego as in obca_params: rectangle centre
 * pose + R(theta)(off, 0), L = ego[0] + ego[2], W = ego[1] + ego[3], off = L/2 - ego[2]) and convex obstacles
 * {q : A q <= b} given by their rows in edge order (one row: half-plane; two: wedge; three or more: polygon).  Signed
 * distance: Euclidean distance when separated, minus the penetration depth (separating-axis value) when overlapping.
 * Read-only: neither call writes solver or rollout state.  Every argument is checked before the first HIP call; a
 * refused call (OBCA_E_INVAL) has no side effect.  That holds for all four calls below, and so does one more refusal: a
 * batch too large for one launch (one segment of up to 64 lanes per instance or rollout, more than 2^31 - 1 blocks of
 * 256 lanes) returns OBCA_E_INVAL.  Asynchronous on hip_stream.
 *
 * Plan clearance of obca_solve_batch outputs.  ego and m (n_obs entries, 1..OBCA_MAX_EDGES) are HOST pointers; the
 * rest DEVICE pointers in obca_solve_batch's shapes: x [B,3,N+1], A [B,N+1,M,2], b [B,N+1,M], variant [B] or NULL.
 * Where variant[b] == 4 every stage is measured against stage 0's rows (what obca_mpc4 reads); otherwise stage k
 * against its own rows.  Outputs: min_clear [B], arg_stage [B], arg_obst [B] (ties to the lowest stage, then the
 * lowest obstacle), stage_obst [B,N+1,n_obs] or NULL.  A (stage, obstacle) pair whose pose, rows or distance is not
 * finite measures NaN, and NaN ranks below every number: min_clear is then NaN, arg_stage / arg_obst the first such pair. */
int obca_plan_clearance(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                        const int32_t* variant, const double* x, const double* A, const double* b,
                        double* min_clear, int32_t* arg_stage, int32_t* arg_obst, double* stage_obst,
                        int32_t device, void* hip_stream);

/* Swept audit of obca_solve_batch outputs (obca_mpc 0.9): the plan between its knots.  Arguments, shapes and the host /
 * device split as obca_plan_clearance.  Interval s (0 <= s < N) joins stage s to stage s + 1; n_sub + 1 samples, both
 * knots included, are measured at the fractions t = j / n_sub (n_sub = 1: the knots only).  The pose is interpolated
 * linearly in (x, y, theta); obstacle rows entry by entry, A(t) = A_s + t (A_s+1 - A_s), b likewise -- exact for a set that
 * translates at constant velocity (the harness's boxes, obca_moving_rows_batch's rectangles); the knots use the stages'
 * own words.  Where variant[b] == 4 every sample is measured against stage 0's rows.  Outputs (DEVICE, [B] unless noted):
 *   min_clear        smallest sample;  arg_interval / arg_obst: its interval and obstacle (ties to the lowest interval,
 *                    then the lowest obstacle: a minimum on the knot shared by intervals s and s + 1 reports s)
 *   lower_bound      certified lower bound of the signed distance over the continuous interpolated motion: min over
 *                    sub-intervals of min((d_j-1 + d_j - delta) / 2, d_j-1, d_j), delta = |dp| + r_max |dtheta| of the
 *                    sub-interval + the largest |dc_i| / n_sub, dc_i = the least-squares (minimum-norm) solution of
 *                    A_s,i dc = b_s+1,i - b_s,i.  Certified for translating obstacles only: NaN when some obstacle's A
 *                    changes by more than 1e-9 max |A_s,i| or the residual exceeds 1e-9 (1 + max |b|) in some interval
 *                    (derivation in csrc/obca_audit_core.h)
 *   first_collision  first interval with a sample < 0, or -1
 *   interval_min     [B,N] or NULL: smallest sample per interval
 * NaN as in obca_plan_clearance: a sample whose pose, rows or distance is not finite measures NaN and NaN ranks below
 * every number, in min_clear (arg_interval the first interval touching it), interval_min and lower_bound.
 * 1 <= n_sub <= 65536; otherwise the checks of obca_plan_clearance. */
int obca_plan_sweep(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                    const int32_t* variant, const double* x, const double* A, const double* b, int32_t n_sub,
                    double* min_clear, double* lower_bound, int32_t* arg_interval, int32_t* arg_obst,
                    int32_t* first_collision, double* interval_min /* [B,N] or NULL */,
                    int32_t device, void* hip_stream);

/* Clearance repair of obca_solve_batch outputs (obca_mpc 0.11): one round of "measure, grow the rows where the plan comes
 * too close, say which instances to solve again".  Arguments, shapes, the host / device split and the checks as
 * obca_plan_sweep; status [B] is obca_solve_batch's.  For every instance with variant != 0 and status 0 or 1, every interval
 * s and obstacle i, d[s,i] is the smallest of obca_plan_sweep's n_sub + 1 samples against that obstacle alone (certified = 1:
 * the obstacle's own certified bound over the interval, NaN where its rows turn), always against A / b as given.  Then
 *   need[s,i]  = gain (target - d[s,i]) where d[s,i] < target, else 0
 *   grow[k,i]  = min(grow_max, grow[k,i] + max(need[k-1,i], need[k,i])) over the intervals that exist; where variant == 4
 *                the largest need[.,i] at every stage (obca_mpc4 reads stage 0's rows only).  In/out, [B,N+1,n_obs],
 *                metres; never decreases.  Zero it before the first round.
 *   b_out[k,r] = b[k,r] + grow[k,i] hypot(A[k,r,0], A[k,r,1]) for every row r of obstacle i: the offset polygon contains the
 *                obstacle grown by a disc of radius grow[k,i], so a knot that keeps dmin from the rows (A, b_out) keeps
 *                dmin + grow[k,i] from the obstacle itself.  Solve again with b_out in place of b; A is not changed.
 *   variant_out[b] = variant[b] if some grow[b,.,.] rose in this call, else 0: passed to obca_solve_batch as its variant it
 *                re-solves exactly the instances whose rows changed and leaves the outputs of the others untouched.
 *   min_clear  [B] or NULL: the smallest d[s,i] of the instance.
 * Passed through -- grow untouched, b_out = b + grow |a| as it stood, variant_out = 0 --: variant 0 and a status outside
 * {0, 1} (not measured, min_clear NaN), and an instance one of whose measurements is not finite (min_clear NaN, the NaN rule
 * of obca_plan_clearance).  b_out must not alias b (it holds intermediate values during the call).  n_sub as
 * obca_plan_sweep, certified 0 or 1, target finite, 0 < gain <= 8, 0 <= grow_max <= 2; variant, status, grow, b_out and
 * variant_out must not be NULL. */
int obca_plan_tighten(const double ego[4], int32_t n_obs, const int32_t* m, int32_t N, int32_t B,
                      const int32_t* variant, const int32_t* status,
                      const double* x, const double* A, const double* b,
                      int32_t n_sub, int32_t certified, double target, double gain, double grow_max,
                      double* grow /* [B,N+1,n_obs], in/out */, double* b_out /* [B,N+1,M] */,
                      int32_t* variant_out /* [B] */, double* min_clear /* [B] or NULL */,
                      int32_t device, void* hip_stream);

/* Rollout audit from the handle's own device state (after obca_rollouts_reset; ego and dmin of that reset).  Rollout
 * b has the knots x_closed[b, 0..steps[b]]; interval s joins knot s to s + 1 (steps[b] == 0: knot 0 alone).  Within
 * an interval the pose is interpolated linearly in (x, y, theta) and n_sub + 1 >= 2 samples, both knots included, are
 * measured (n_sub = 1: the knots only).  Obstacles: the static rows of the reset and EVERY present moving box, sensed
 * or not, at its recorded position (dyn_hist), moving linearly with heading and size fixed within an interval; the
 * unrecorded last knot takes the harness's update law (advance by T_closed[s] * speed along the heading, appear at
 * k == t_start); a box that appears at knot s + 1 counts from that knot on.  Obstacle indices: static i, then
 * n_static + j for moving box j.  Outputs (DEVICE, [B] unless noted):
 *   min_clear        smallest sampled signed distance;  arg_step / arg_obst: its interval and obstacle (lowest first)
 *   lower_bound      certified lower bound of the signed distance over the continuous interpolated motion:
 *                    min over sub-intervals of (d_j + d_j+1 - delta) / 2 with delta = |dp| + r_max |dtheta| + the
 *                    largest |dc| of a moving box (r_max: pose point to farthest footprint corner; derivation in
 *                    csrc/obca_audit_core.h)
 *   first_collision  first interval with a sampled distance < 0, or -1
 *   first_violation  first knot with a distance < dmin - 1e-6, or -1
 *   step_min         [B,max_steps] or NULL: smallest sample per interval (+inf beyond the rollout's intervals) */
int obca_rollouts_audit(obca_rollouts* r, int32_t n_sub,
                        double* min_clear, double* lower_bound, int32_t* arg_step, int32_t* arg_obst,
                        int32_t* first_collision, int32_t* first_violation,
                        double* step_min, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Obstacle rows of moving rectangles for obca_solve_batch, built on the device: what the closed loop's harness writes
 * for its sensed boxes (exact sensing), for callers that solve batches directly.  Per instance and horizon stage
 * kk = 0..N the Ms static rows are copied and every box gets the four rows of obca_rollouts_set_swept_rows' rectangle
 * (half_window = margin = 0: the box itself at stage kk, the harness's words).  DEVICE pointers: static_A [B,Ms,2],
 * static_b [B,Ms] (may be NULL when Ms = 0), boxes [B,n_box,13] -- the tuple of obca_rollouts_reset's dyn: centre now
 * 0, 1; length 3, width 4; speed 5; cos / sin of the heading 11, 12 -- and Ts [B], the step length of the solve (both may
 * be NULL when n_box = 0); outputs A [B,N+1,Ms + 4 n_box,2], b [B,N+1,Ms + 4 n_box].  static_A and A must be 16-byte
 * aligned (hipMalloc's are).  N >= 1, B >= 1, 0 <= Ms <= 32, 0 <= n_box <= 8, Ms + 4 n_box >= 1, half_window in [0, 1],
 * margin in [0, 2].  Every argument is checked before the first HIP call; a refused call (OBCA_E_INVAL) has no side
 * effect.  Asynchronous on hip_stream. */
int obca_moving_rows_batch(int32_t B, int32_t N, int32_t Ms, int32_t n_box, const double* static_A, const double* static_b,
                           const double* boxes, const double* Ts, double half_window, double margin, double* A, double* b,
                           int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Refinement between the two stages of the open-loop planner (obca_mpc 0.12), on the device: stage 1's free-time plans in,
 * stage 2's reference, step and variant mask out (the reference's closedLoop.update_path with allAviable = 1, src/closed_loop.py:567-589).
 * DEVICE pointers: x [B,3,N+1], ts [B] and status [B] are obca_solve_batch's xopt, ts_opt and status (status NULL: every
 * instance counts as feasible).  With N2 = ratio N, per instance:
 *   xref_out [3,N2+1]  point j < N2, i = j / ratio, q = j % ratio: (double)q * ((x[i+1] - x[i]) / (double)ratio) + x[i] in
 *                      x and y, multiply and add rounded separately (numpy's linspace without its endpoint, word for word);
 *                      point N2 is knot N; yaw_j = atan2(py_j+1 - py_j, px_j+1 - px_j), yaw_N2 = yaw_N2-1
 *   ts_out             ((double)N * ts) / (double)N2
 *   variant_out        variant_ok: what obca_solve_batch is to run for stage 2 (variant_out may be NULL)
 * Passed through -- variant_out = 0, every point of xref_out = knot 0 of the plan (zeros where that knot is not finite),
 * ts_out = ts / ratio where ts is finite, else 0 --: a status outside {0, 1}, a knot or a difference of neighbouring
 * positions that is not finite, ts not finite or <= 0.  No output is ever NaN, so that the launches that follow (the
 * rows builder, the masked solve) read numbers throughout.
 * B >= 1, N >= 1, ratio >= 1, ratio N <= 127 (the longest horizon of obca_dims), variant_ok 4, 6 or 8; x, ts, xref_out and
 * ts_out not NULL.  Every argument is checked before the first HIP call; a refused call (OBCA_E_INVAL) has no side
 * effect.  Asynchronous on hip_stream. */
int obca_plan_refine(int32_t B, int32_t N, int32_t ratio, const double* x, const double* ts,
                     const int32_t* status /* [B] or NULL */, int32_t variant_ok,
                     double* xref_out /* [B,3,ratio N+1] */, double* ts_out /* [B] */,
                     int32_t* variant_out /* [B] or NULL */, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * From a route to the reference of a fixed-horizon solve (obca_mpc 0.13), on the device: the two steps around
 * obca_astar_batch that make the open-loop planner hierarchical -- map, dilated map, route, reference.
 *
 * Disk dilation of B occupancy grids (the reference's mapModel.dilate_map, src/model_map.py:103-107).  DEVICE pointers
 * grid and out, [B,rows,cols] uint8:
 *   out[b,r,c] = 1 iff some cell (r + dy, c + dx) inside the grid with dy^2 + dx^2 <= level^2 is non-zero in grid[b], else 0.
 * Cells outside the grid count as free; any non-zero input byte counts as occupied; level 0 copies (a non-zero byte becomes
 * 1).  The output is what obca_astar_batch takes.  B, rows, cols >= 1, rows*cols <= 65535 (obca_astar_batch's bound),
 * 0 <= level <= 16 (a lane reads at most (2 level + 1)^2 = 1089 bytes; a car of the reference is under 4 cells long),
 * grid and out not NULL and not overlapping (grid == out included).  Every argument is checked before the first HIP call;
 * a refused call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
int obca_grid_dilate_batch(const uint8_t* grid, int32_t B, int32_t rows, int32_t cols, int32_t level, uint8_t* out,
                           int32_t device, void* hip_stream);

/* Routes resampled to N + 1 knots equally spaced in arc length.  DEVICE pointers: path [B,3,path_max] and path_len [B] as
 * obca_astar_batch writes them (negative codes included; the yaw row is read only for the fill below), start [B,3] and
 * goal [B,3] poses to pin the ends to (either may be NULL); outputs xref_out [B,3,N+1] (obca_solve_batch's xref) and
 * ok_out [B].  For an instance with L = path_len >= 2 points p_i, every operation rounded on its own (no FMA):
 *   d_i = sqrt(dx_i dx_i + dy_i dy_i), i = 0 .. L-2;  S_0 = 0, S_i+1 = S_i + d_i in index order;  S = S_L-1
 *   knot k < N  s_k = ((double)k S) / (double)N; its segment is the first i with d_i > 0 and S_i+1 >= s_k;
 *               t = (s_k - S_i) / d_i;  p = p_i + t (p_i+1 - p_i) per coordinate
 *   knot N      the last route point itself
 *   pins        the position of knot 0 becomes start[0..1], that of knot N goal[0..1], where given
 *   yaw_k       atan2(y_k+1 - y_k, x_k+1 - x_k) on these final positions for k < N, yaw_N = yaw_N-1 (the rule of
 *               create_reference_path, src/a_star.py:189-200); then yaw_0 = start[2], yaw_N = goal[2] where given
 *   ok_out      1
 * Not resampled, ok_out = 0: path_len < 2 or > path_max, a point (x, y or yaw) among the first path_len that is not finite
 * (points beyond path_len are never read), S zero or not finite, a given start or goal pose that is not finite (it is
 * dropped for that instance).  Such an instance gets, where start and goal are both given and finite, start at knot 0 and
 * goal at knots 1 .. N, all three components (the start/goal-only reference); otherwise point 0 of its path at every knot,
 * or zeros where that point is not finite.  No output is ever NaN.
 * B >= 1, path_max >= 1, 1 <= N <= 127 (the longest horizon of obca_dims); path, path_len, xref_out and ok_out not NULL.
 * Every argument is checked before the first HIP call; a refused call (OBCA_E_INVAL) has no side effect.  Asynchronous on
 * hip_stream. */
int obca_route_resample(int32_t B, int32_t path_max, int32_t N, const double* path, const int32_t* path_len,
                        const double* start /* [B,3] or NULL */, const double* goal /* [B,3] or NULL */,
                        double* xref_out /* [B,3,N+1] */, int32_t* ok_out /* [B] */, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Scene pools (obca_mpc 0.14), on the device: which obstacles of a pool of up to 64 a solve sees.  OBCA_MAX_OBST bounds what
 * one solve reads, not what a world holds: this call scores every obstacle of a pool by its distance to a set of poses, takes
 * the n_sel nearest and gathers their rows for obca_solve_batch; called again with the plans solved against that selection it
 * keeps a running minimum per obstacle, so that an obstacle left out which a plan comes close to is taken in.
 * ego is a HOST pointer, the rest DEVICE pointers.  One pool per instance: K convex obstacles of exactly E rows each,
 *   pool_A [B,K,E,2], pool_b [B,K,E], pool_v [B,K,2] in m/s or NULL (nothing moves), Ts [B] (may be NULL when pool_v is).
 * Obstacle i at horizon stage kk has the rows A and b_kk[r] = b[r] + (kk * Ts) * (A[r,0] v_x + A[r,1] v_y), every product and
 * sum rounded on its own (no FMA) -- exact for a set that translates at constant velocity, the fact obca_plan_sweep rests on.
 * Poses: x [B,3,N+1] (a reference window, later obca_solve_batch's xopt) and x0 [B,3] or NULL (one more sample, against
 * stage 0's rows: the car's pose is not knot 0 of a window).  The score of obstacle i is the smallest signed distance
 * between the car footprint and the obstacle (the distance of obca_plan_clearance) over the samples: x0, and per interval
 * stage s -> s + 1 the n_sub + 1 samples of obca_plan_sweep (n_sub = 1: the knots only; pose and b interpolated linearly),
 * stage kk's pose against stage kk's rows; where variant[b] == 4 every sample against stage 0's rows (what obca_mpc4 reads).
 * A sample whose pose is not finite is skipped.  variant [B] or NULL (every instance 6), status [B] or NULL (every instance 0).
 *   accumulate = 0   score [B,K] is written from the samples; every usable instance counts as changed
 *   accumulate = 1   score is in/out and becomes min(score, this call's samples); sel is in/out.  Only instances with
 *                    variant != 0 and status 0 or 1 (obca_solve_batch's) are measured; the others keep score and selection
 *   min_clear        [B] or NULL: THIS call's smallest distance over all K obstacles (no running minimum); NaN where the
 *                    instance was not measured
 *   sel [B,n_sel]    the n_sel obstacles with the smallest score, ties to the lower pool index, listed in ascending pool
 *                    index (slots do not flip when two scores cross; comparing selections is an element-wise compare)
 *   variant_out [B]  variant[b] where the selection differs from the one passed in (always with accumulate = 0), else 0:
 *                    as obca_solve_batch's variant it re-solves exactly the instances whose rows changed (obca_plan_tighten's idiom)
 *   A_out, b_out     [B,N+1,n_sel E,2] and [B,N+1,n_sel E]: obca_solve_batch's rows for a handle with m = E, n_sel times;
 *                    written for every instance, changed or not
 *   ok_out [B]       1, or 0 for an unusable instance: a pool row, a velocity or a Ts it needs that is not finite, a pool
 *                    row a = (0, 0), no sample pose that is finite, a distance that is no number (overflow), or (accumulate,
 *                    not measured) a selection passed in that is not an ascending list of pool indices.  Such an instance gets
 *                    variant_out 0, sel = 0 .. n_sel-1, score untouched, min_clear NaN and every output row a = (1, 0),
 *                    b = -1e6.  No row, score or selection written is ever NaN: masked launches downstream read numbers.
 * B >= 1, 1 <= K <= 64 (one lane per obstacle), 1 <= E <= OBCA_MAX_EDGES, 1 <= N <= 127, 1 <= n_sel <= min(K, OBCA_MAX_OBST),
 * 1 <= n_sub <= 256, accumulate 0 or 1, ego finite; Ts not NULL where pool_v is given; A_out 16-byte aligned (hipMalloc's
 * are); ego, pool_A, pool_b, x, score, sel, A_out, b_out, variant_out and ok_out not NULL.  Every argument is checked before
 * the first HIP call; a refused call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
int obca_scene_select(const double ego[4], int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub,
                      int32_t accumulate, const double* pool_A, const double* pool_b, const double* pool_v /* or NULL */,
                      const double* Ts /* [B] */, const double* x, const double* x0 /* [B,3] or NULL */,
                      const int32_t* variant /* [B] or NULL */, const int32_t* status /* [B] or NULL */,
                      double* score /* [B,K] */, int32_t* sel /* [B,n_sel] */, double* A_out, double* b_out,
                      int32_t* variant_out /* [B] */, int32_t* ok_out /* [B] */, double* min_clear /* [B] or NULL */,
                      int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Occupancy grids to scene pools (obca_mpc 0.15), on the device: the inverse of obca_rasterise_batch.  Every grid
 * [rows,cols] of bytes (non-zero = occupied) is covered by disjoint axis-parallel rectangles of cells, and every rectangle
 * becomes one pool obstacle of 4 rows for obca_scene_select: pool_A [B,K,4,2], pool_b [B,K,4].  All pointers are DEVICE pointers.
 * Cover (greedy right-then-down; csrc/obca_gridpool_core.h holds the serial definition the kernel reproduces exactly):
 *   work = occupied cells; n = 0
 *   for r = 0 .. rows-1, for c = 0 .. cols-1 (row-major): if (r, c) in work:
 *       c1 = last column of the unbroken run of work cells (r, c), (r, c+1), ...
 *       r1 = last row such that every cell of rows r .. r1, columns c .. c1 is in work
 *       remove rows r..r1 x columns c..c1 from work;  if n < K: rect[n] = (r, c, r1, c1);  n = n + 1
 *   count = n                      (the true number, also where it exceeds K)
 * The rectangles are disjoint, their union is the occupied set, they are listed in strictly ascending (r0, c0).  No
 * minimum-count cover.
 * Rows of rectangle (r0, c0, r1, c1): xlo = c0 resolution - pad, xhi = c1 resolution + pad, ylo = r0 resolution - pad,
 * yhi = r1 resolution + pad, every product and difference rounded on its own (no FMA); E = 4 rows in the order
 * (0, 1 | yhi), (1, 0 | xhi), (0, -1 | -ylo), (-1, 0 | -xlo) -- for a rectangle with area what obstacle_H_Represent gives
 * for the clockwise polygon [[xlo,yhi],[xhi,yhi],[xhi,ylo],[xlo,ylo],[xlo,yhi]].  pad = 0: a cell is a lattice point (the
 * reference's convention; the boxes rasterise back to exactly these cells at the same resolution); pad = resolution / 2: a
 * cell is a square centred on its lattice point, so that neighbouring rectangles touch.
 *   rect [B,K,4]     or NULL: (r0, c0, r1, c1) of slot k, (-1,-1,-1,-1) for a spare slot
 *   count [B]        the number of rectangles of the cover, also where it exceeds K
 *   ok [B]           1 if count <= K, else 0: the first K rectangles are written and valid, the map is not covered
 *   spare slots      k >= count: the rows of the unit square [-far-1, -far]^2 in the same row order.  far is the caller's
 *                    choice because a spare that is selected becomes rows of a solve: 100 or 1000 leave the structured solver's
 *                    plans as they are, 1e6 (the fill of obca_scene_select) makes it fail (csrc/obca_gridpool_core.h)
 * Nothing written is ever NaN.
 * B >= 1, 1 <= K <= 64, rows >= 1, cols >= 1, rows * ceil(cols / 64) <= 4096 (the bit-packed grid in 32 KB of LDS: 11 x 40,
 * 255 x 255 and 1024 x 256 fit), resolution > 0, pad >= 0 and far > 0, all finite; grid, pool_A, pool_b, count and ok not
 * NULL; pool_A 16-byte aligned (hipMalloc's are); device >= 0.  Every argument is checked before the first HIP call; a refused
 * call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
int obca_grid_pool(const uint8_t* grid /* [B,rows,cols] */, int32_t B, int32_t rows, int32_t cols, int32_t K,
                   double resolution, double pad, double far,
                   double* pool_A /* [B,K,4,2] */, double* pool_b /* [B,K,4] */, int32_t* rect /* [B,K,4] or NULL */,
                   int32_t* count /* [B] */, int32_t* ok /* [B] */, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Closed loop over scene pools (obca_mpc 0.16), on the device: the harness between two solves of a receding-horizon loop
 * whose world is a pool (obca_scene_select's: K <= 64 obstacles of E rows, optionally translating).  One step of the loop is
 * three calls on one stream: obca_scene_select (the pool as it is now, the window and pose below, variant_out as its variant),
 * obca_solve_batch (its rows), then this call with solved = 1.  It has no handle: the state is the caller's buffers, named by
 * one descriptor.  csrc/obca_poolloop_core.h holds the serial definition the kernel reproduces word for word.
 *
 * solved = 1, for every rollout with flags[b] == OBCA_RUN (the others keep every word of state and history), kb = k[b]:
 *   record    status_hist[b,kb] = status[b], iters_hist[b,kb] = iters[b], sel_hist[b,kb,:] = sel[b,:]
 *   read      p1 = xopt[b,:,1], u = uopt[b,:,0], ts = ts_opt[b].  A status outside {0, 1}, a word of p1, u or ts that is not
 *             finite, or ts <= 0: flags[b] = OBCA_DONE_FAILED and nothing else is written (the failed step counts in no
 *             other history: obca_rollouts_step's rule)
 *   measure   (n_sub > 0) c = the smallest signed distance between the car and ANY of the K obstacles over the applied
 *             interval: obca_scene_select's samples (n_sub + 1 per interval, pose and rows interpolated) of the two-knot plan
 *             [x0[b], p1] with Ts = ts, an obstacle with a velocity moving from its rows now to its rows ts later.  c NaN:
 *             OBCA_DONE_FAILED, nothing else written; otherwise clear_hist[b,kb] = c
 *   move      (pool_v given) pool_b[b,i,r] += ts * (A[r,0] v_x + A[r,1] v_y), the words of obca_scene_select's stage 1: the
 *             pool accumulates the applied step lengths, it is not b0 + t_total (a . v)
 *   advance   x0 = p1, u0 = u, x_closed[b,kb+1] = p1, u_closed[b,kb] = u, T_closed[b,kb] = ts, k[b] = kb + 1
 *   flag      n_sub > 0 and c < clearance: OBCA_DONE_COLLISION (the colliding step stays in the history, as with
 *             obca_rollouts_set_collision_stop); else kb + 1 == max_steps: OBCA_DONE_CAP; else the car within
 *             sqrt(goal_tol2) of goal[b] (!(dx dx + dy dy >= goal_tol2), obca_rollouts_step's test with its 0.1):
 *             OBCA_DONE_GOAL
 * solved = 0 starts every rollout; the caller has put the start poses into x0 and the pools' rows into pool_b: k = 0, u0 = 0,
 *   x_closed[b,0] = x0[b] and NaN beyond, u_closed, T_closed, status_hist, iters_hist 0, clear_hist +inf, sel_hist -1;
 *   flags[b] = OBCA_DONE_FAILED for a pose that is not finite or a path_len[b] outside 1 .. path_max, else OBCA_DONE_GOAL
 *   for a start at the goal, else OBCA_RUN.  The solve's pointers are not read and may be NULL.
 * Then, always: for a rollout that is OBCA_RUN variant_out[b] = variant and xref_out[b] = the N + 1 path points from the one
 *   nearest to the car on (the first strict minimum of the squared distance below 1e5 over path[b,:,0 .. path_len[b]-1],
 *   point 0 when there is none; the last point repeated beyond the route's end: obca_rollouts_step's window); for every other
 *   rollout variant_out[b] = 0 and every column of xref_out[b] is x0[b] (0 for a word that is not finite), so that the masked
 *   launches downstream read numbers.  Nothing written is NaN except the fill of x_closed.
 * B >= 1, 1 <= K <= 64, 1 <= E <= OBCA_MAX_EDGES, 1 <= N <= 127, path_max >= 1, 1 <= max_steps <= 1024, solved 0 or 1,
 * variant 4, 6 or 8, 0 <= n_sub <= 256, 0 <= n_sel <= OBCA_MAX_OBST (n_sel >= 1 needs sel and sel_hist), clearance and ego
 * finite (to measure without stopping pass a clearance no distance reaches, e.g. -1e300), goal_tol2 > 0 and finite,
 * struct_size == sizeof(obca_pool_loop), device >= 0; every pointer not marked "or NULL" not NULL, the solve's only with
 * solved = 1.  State the caller broke forms no address outside its buffers: a RUN rollout whose k[b] is outside
 * 0 .. max_steps-1 ends OBCA_DONE_FAILED with nothing else written, and a path_len[b] outside 1 .. path_max is clamped to
 * that range where the window reads the path (a start makes such a rollout OBCA_DONE_FAILED).  Words: the window search and
 * the goal test round every product and sum on their own; the clearance is obca_scene_select's arithmetic as the library
 * builds it (contracted products, the device's sin / cos), so clear_hist equals obca_scene_select's min_clear on the same
 * device word for word and a host evaluation only where the arithmetic is exact.  Every argument is checked before the first HIP call; a refused call (OBCA_E_INVAL) has no side effect.
 * Asynchronous on hip_stream. */
typedef struct obca_pool_loop {
    uint32_t struct_size;              /* sizeof(obca_pool_loop): set by obca_pool_loop_init() */
    uint32_t reserved_;
    int32_t B, K, E, N, n_sel, path_max, max_steps, variant, n_sub;
    int32_t reserved2_;
    double clearance, goal_tol2;       /* obca_pool_loop_init: -1e300 (never stops) and 0.1 */
    double ego[4];                     /* obca_pool_loop_init: 1.7, 0.75, 1.7, 0.75 (obca_params.ego's default) */
    /* read-only */
    const double* pool_A;              /* [B,K,E,2] */
    const double* pool_v;              /* [B,K,2] or NULL */
    const double* goal;                /* [B,2] */
    const double* path;                /* [B,3,path_max] */
    const int32_t* path_len;           /* [B] */
    /* the solve (solved = 1) */
    const int32_t* status;             /* [B] */
    const int32_t* iters;              /* [B] */
    const double* ts_opt;              /* [B] */
    const double* xopt;                /* [B,3,N+1] */
    const double* uopt;                /* [B,2,N] */
    const int32_t* sel;                /* [B,n_sel], or NULL with n_sel = 0 */
    /* state, in and out */
    double* x0;                        /* [B,3] */
    double* u0;                        /* [B,2] */
    double* pool_b;                    /* [B,K,E] */
    int32_t* k;                        /* [B] */
    int32_t* flags;                    /* [B] */
    /* history, S = max_steps */
    double* x_closed;                  /* [B,S+1,3] */
    double* u_closed;                  /* [B,S,2] */
    double* T_closed;                  /* [B,S] */
    int32_t* status_hist;              /* [B,S] */
    int32_t* iters_hist;               /* [B,S] */
    double* clear_hist;                /* [B,S] */
    int32_t* sel_hist;                 /* [B,S,n_sel], or NULL with n_sel = 0 */
    /* outputs: the next solve's window and variant */
    double* xref_out;                  /* [B,3,N+1] */
    int32_t* variant_out;              /* [B] */
} obca_pool_loop;

/* zero-fills *d and sets struct_size, clearance, goal_tol2 and ego: the one way to start filling an obca_pool_loop */
void obca_pool_loop_init(obca_pool_loop* d);
int obca_pool_loop_advance(const obca_pool_loop* d, int32_t solved, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Fleet closed loop (obca_mpc 0.18), on the device: V cars that share one world avoid each other.  A fleet is G worlds of V
 * cars; rollout b = g V + a of a closed loop over scene pools (above) is car a of world g, B = G V.  Every rollout's pool has
 * K = Ks + V slots of E = 4 rows: slots 0 .. Ks-1 are the caller's obstacles and are never touched here, slot Ks + j is "car j
 * of my world".  The fleet's time is synchronous: the loop runs obca_mpc8 with one Ts per world.  One step of the loop is the
 * three calls of obca_pool_loop_advance's recipe (after a copy of x0 to x_prev) and then this call with measure = 1 and
 * step = the loop step just applied; a start is obca_pool_loop_advance(solved = 0), then this call with measure = 0.  It has
 * no handle; csrc/obca_fleet_core.h holds the serial definition the kernel reproduces.
 *
 * measure = 1 and n_sub > 0, for every car that applied a step in this loop step (k[b] == step + 1):
 *   measure   c = the smallest signed distance to every OTHER car of its world over the interval, at n_sub + 1 samples with
 *             both poses interpolated linearly (obca_plan_sweep's samples): obca_plan_clearance's distance between the
 *             footprint of the car of lower index and the rows of the car of higher index (no margin), so that both cars of
 *             a pair read one word; folded in ascending index of the other car.  A car that stepped moves from x_prev[b] to
 *             x0[b]; one that did not stands at x0[b].  A pair with a pose word that is not finite is not measured (+inf).
 *             `see` does not enter: a car is hit by whoever is there.
 *   record    agent_clear_hist[b,step] = c (not written when c is NaN: a distance that overflowed)
 *   flag      c NaN: OBCA_DONE_FAILED; c < clearance and flags[b] == OBCA_RUN: OBCA_DONE_COLLISION (a car that has just reached
 *             its goal keeps OBCA_DONE_GOAL; its distance is recorded all the same).  A car flagged here gets variant_out[b] = 0
 *             and every column of xref_out[b] = x0[b] (0 for a word that is not finite): obca_pool_loop_advance's rule for
 *             masked launches.  A car that did not step gets no history word and keeps its flag.
 * Then, always, from the flags as they are now, for every rollout (g, a) and every j < V:
 *   spare     j == a, or see == OBCA_FLEET_SEE_LOWER and j > a (prioritised planning: a car yields only to lower indices), or a
 *             word of car j's pose that is not finite: the rows of the unit square [-far-1, -far]^2 (obca_grid_pool's spare,
 *             for its reason) and v = 0
 *   car j     otherwise pool_A / pool_b[b,Ks+j] = the rectangle of car j at x0[g V + j] (obca_plan_clearance's footprint:
 *             L = ego0 + ego2, W = ego1 + ego3, centre off = L/2 - ego2 ahead of the pose point) grown by margin, as four
 *             unit rows in obca_grid_pool's order: (-sin, cos | n.c + W/2 + margin), (cos, sin | n.c + L/2 + margin) and the
 *             two negated normals; every product and sum rounded on its own (no FMA), no -0.0 in A, so that heading 0 gives
 *             the words of the axis-parallel box.  pool_v[b,Ks+j] = s (cos, sin) with s = u0[g V + j, 0] if
 *             predict == OBCA_FLEET_PREDICT_VELOCITY and flags[g V + j] == OBCA_RUN, else 0: a car that has ended is parked
 *             where it stands and stays an obstacle.
 * Nothing written is ever NaN.
 * G >= 1, 1 <= V <= 16, Ks >= 0, Ks + V <= 64, 1 <= N <= 127, 0 <= step < max_steps <= 1024, 0 <= n_sub <= 256 (0: not
 * measured), measure 0 or 1, see and predict each one of their two values, clearance finite (-1e300: measured, never stopped),
 * margin >= 0, far > 0 and ego finite, struct_size == sizeof(obca_fleet), device >= 0, no pointer NULL.  Every argument is
 * checked before the first HIP call; a refused call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
#define OBCA_FLEET_SEE_ALL 0           /* every other car of the world is an obstacle */
#define OBCA_FLEET_SEE_LOWER 1         /* only the cars of lower index are */
#define OBCA_FLEET_PREDICT_VELOCITY 0  /* a running car translates with its last applied speed along its heading */
#define OBCA_FLEET_PREDICT_STATIC 1    /* every car stands where it is */
typedef struct obca_fleet {
    uint32_t struct_size;              /* sizeof(obca_fleet): set by obca_fleet_init() */
    uint32_t reserved_;
    int32_t G, V, Ks, N, max_steps, step, n_sub, see, predict;
    int32_t reserved2_;
    double clearance, margin, far;     /* obca_fleet_init: -1e300 (never stops), 0 and 100 */
    double ego[4];                     /* obca_fleet_init: 1.7, 0.75, 1.7, 0.75 (obca_params.ego's default) */
    /* read-only, B = G V */
    const double* x_prev;              /* [B,3] the poses before the step */
    const double* x0;                  /* [B,3] the poses now */
    const double* u0;                  /* [B,2] the last applied inputs */
    const int32_t* k;                  /* [B] */
    /* in and out */
    int32_t* flags;                    /* [B] */
    double* pool_A;                    /* [B,K,4,2], K = Ks + V: slots Ks .. K-1 written */
    double* pool_b;                    /* [B,K,4] */
    double* pool_v;                    /* [B,K,2] */
    double* agent_clear_hist;          /* [B,max_steps] */
    double* xref_out;                  /* [B,3,N+1] */
    int32_t* variant_out;              /* [B] */
} obca_fleet;

/* zero-fills *d and sets struct_size, clearance, far and ego: the one way to start filling an obca_fleet */
void obca_fleet_init(obca_fleet* d);
int obca_fleet_step(const obca_fleet* d, int32_t measure, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Fleet closed loop, prediction by plans (obca_mpc 0.19), on the device.  obca_fleet_step predicts another car as a rectangle
 * that translates at its last speed; the N-stage plan that car has just solved says where it will be, and how it will be
 * turned, at exactly the stage times of the other cars' next solves.  Two calls: obca_fleet_tracks turns the plans just applied
 * into rows per stage (a track per car), obca_scene_select_staged is obca_scene_select with such rows for the last Kt slots.
 * One step of the loop: obca_scene_select_staged (Kt = V, stage_group = V, the tracks and track_ok of the last step),
 * obca_solve_batch, obca_pool_loop_advance, obca_fleet_step (OBCA_FLEET_PREDICT_VELOCITY: the pool slots stay the velocity
 * prediction, the fallback for a car without a usable plan and what obca_pool_loop_advance's clearance measures), then
 * obca_fleet_tracks with the solve just applied.  A start zeroes track_ok.
 *
 * obca_fleet_tracks, B = G V, car j of world g is rollout q = g V + j:
 *   usable plan   flags[q] == OBCA_RUN, k[q] == step + 1 (the car applied this loop step), status[q] 0 or 1, and all
 *                 3 (N + 1) words of xopt[q] finite
 *   stage poses   the next solve starts one step later, so its stage kk is knot kk + 1 of this plan: xopt[q,:,kk+1] for
 *                 kk < N; for kk = N the position x_N + (x_N - x_N-1) (each operation rounded on its own) with the heading of
 *                 knot N
 *   track         track_A / track_b[g,j,kk] = the four rows obca_fleet_step writes for a car at that pose (its rectangle
 *                 grown by margin).  obca_pool_loop_advance copied knot 1 to x0, so stage 0 holds the words of the pool slot.
 *                 Without a usable plan every stage holds the rows at x0[q], or the spare's where that pose is not finite.
 *   track_ok      [B,V]: track_ok[g V + a, j] = 1 where the plan of car j is usable and slot Ks + j of car a is no spare
 *                 (obca_fleet_step's rule: j == a, see == OBCA_FLEET_SEE_LOWER and j > a, a pose word that is not finite)
 * Nothing written is NaN as long as the rows of the poses are finite (poses below 1e150 m).  G >= 1, 1 <= V <= 16,
 * 1 <= N <= 127, step >= 0, see one of its two values, margin >= 0, far > 0 and ego finite, struct_size ==
 * sizeof(struct obca_fleet_tracks), device >= 0, no pointer NULL.  Every argument is checked before the first HIP call; a refused
 * call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream; csrc/obca_fleet_tracks_core.h is the serial definition. */
struct obca_fleet_tracks {
    uint32_t struct_size;              /* sizeof(struct obca_fleet_tracks): set by obca_fleet_tracks_init() */
    uint32_t reserved_;
    int32_t G, V, N, step, see;
    int32_t reserved2_;
    double margin, far;                /* obca_fleet_tracks_init: 0 and 100 */
    double ego[4];                     /* obca_fleet_tracks_init: 1.7, 0.75, 1.7, 0.75 */
    /* read-only, B = G V, as they are after obca_fleet_step */
    const double* x0;                  /* [B,3] */
    const int32_t* flags;              /* [B] */
    const int32_t* k;                  /* [B] */
    const double* xopt;                /* [B,3,N+1] the solve that was just applied */
    const int32_t* status;             /* [B] */
    /* written */
    double* track_A;                   /* [G,V,N+1,4,2] one track per car per world, shared by its observers */
    double* track_b;                   /* [G,V,N+1,4] */
    int32_t* track_ok;                 /* [B,V] what observer b = g V + a may use of car j */
};   /* no typedef: the call has the descriptor's name, so C and C++ say `struct obca_fleet_tracks` */

/* zero-fills *d and sets struct_size, far and ego: the one way to start filling an obca_fleet_tracks */
void obca_fleet_tracks_init(struct obca_fleet_tracks* d);
int obca_fleet_tracks(const struct obca_fleet_tracks* d, int32_t device, void* hip_stream);

/* obca_scene_select with rows per stage for the last Kt pool slots.  The arguments are obca_scene_select's and
 *   Kt            0 <= Kt <= K
 *   stage_group   >= 1, B % stage_group == 0: instance b reads block b / stage_group (a fleet passes V)
 *   stage_A       [B/stage_group, Kt, N+1, E, 2], stage_b [B/stage_group, Kt, N+1, E], stage_ok [B,Kt]; NULL only with Kt = 0
 * Pool slot K - Kt + t of instance b is staged where stage_ok[b,t] != 0: its rows at stage kk are stage_A / stage_b[b /
 * stage_group, t, kk] and its pool_v plays no part in them (its pool words are still checked).  Every other slot, and a
 * staged slot with stage_ok == 0, behaves exactly as in obca_scene_select.  The samples of a staged slot are the same (x0
 * against stage 0, per interval the n_sub + 1 samples, variant 4: stage 0 at every sample); at sample j of interval s its rows
 * are A and b interpolated entry by entry between stages s and s + 1 (obca_plan_sweep's rule for rows per stage; the distance
 * normalises the slightly shorter normals of a rectangle that turns).  Ranking, sel, variant_out and min_clear are unchanged;
 * a selected staged slot hands its stage rows to A_out / b_out as they are.  Unusable as well: a staged row word that is not
 * finite, a staged row a = (0, 0) at any stage of a slot with stage_ok != 0.  With Kt = 0 or every stage_ok 0 every output is
 * obca_scene_select's word for word, and so it is for a track that holds obca_scene_select's own stage rows. */
int obca_scene_select_staged(const double ego[4], int32_t B, int32_t K, int32_t E, int32_t N, int32_t n_sel, int32_t n_sub,
                             int32_t accumulate, const double* pool_A, const double* pool_b, const double* pool_v /* or NULL */,
                             const double* Ts /* [B] */, const double* x, const double* x0 /* [B,3] or NULL */,
                             const int32_t* variant /* [B] or NULL */, const int32_t* status /* [B] or NULL */, int32_t Kt,
                             int32_t stage_group, const double* stage_A, const double* stage_b, const int32_t* stage_ok,
                             double* score /* [B,K] */, int32_t* sel /* [B,n_sel] */, double* A_out, double* b_out,
                             int32_t* variant_out /* [B] */, int32_t* ok_out /* [B] */, double* min_clear /* [B] or NULL */,
                             int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Closed loop over scene pools, obstacles on timed tracks (obca_mpc 0.20), on the device.  An obstacle of a pool either
 * translates for ever at pool_v or is another car of a fleet; here the last Kt slots of every rollout's pool (K slots of
 * E = 4 rows) follow TRACKS: timed pose sequences (recorded or scripted road users that turn, brake, stop or set off later).
 * Every loop step this call turns the tracks into the rows of those slots now, their chord velocities and their rows at the
 * N + 1 stage times of the next solve -- obca_scene_select_staged's stage_A / stage_b / stage_ok with Kt and stage_group = 1
 * -- and measures what the car really kept from the tracked obstacles over the interval it has just driven.  One step of the
 * loop: a copy of x0 to x_prev, obca_scene_select_staged, obca_solve_batch, obca_pool_loop_advance, then this call with
 * measure = 1 and step = the loop step just applied; a start is obca_pool_loop_advance(solved = 0), then this call with
 * measure = 0.  It has no handle; csrc/obca_pool_tracks_core.h holds the serial definition the kernel reproduces.
 *
 * Bt = B / group track blocks, rollout b reads block b / group; track j of a block is pool slot s = K - Kt + j.
 *   track_state   [B,Kt]: 0 where track_len == 0 (a spare on request); 1 where the track is usable: 1 <= len <= L, the first
 *                 len pose words and times finite, the times strictly increasing, the four size words finite with
 *                 size0 + size2 and size1 + size3 finite and > 0, and the rollout's own time words usable (Ts[b] finite and > 0,
 *                 t0[b] finite); -1 otherwise.  A slot that is not in state 1 is a spare and nothing read from its track
 *                 reaches an output.
 *   pose at t     before t_0, or with one knot: knot 0; at or after the last time: the last knot (the obstacle parks); else
 *                 with i the largest index with t_i <= t (binary search) a = (t - t_i) / (t_i+1 - t_i) and every word is
 *                 w_i + a (w_i+1 - w_i), each operation rounded on its own; t == t_i gives knot i's words.  Headings are
 *                 interpolated as numbers: the caller unwraps them.
 *   times         stage kk of the next solve of rollout b is at t0[b] + (double)(k[b] + kk) Ts[b] (one product, one sum), so
 *                 stage kk now and stage kk - 1 one step later are one word, and so are their rows.
 * measure = 1 and n_sub > 0, for every rollout that applied a step in this loop step (k[b] == step + 1), obca_fleet_step's
 * rules: c = the smallest signed distance, over the n_sub + 1 samples j of the interval, between the car's footprint (ego) at
 *   the pose interpolated between x_prev[b] and x0[b] and the margin-free rectangle of every usable track at the TRACK's pose
 *   at the sample's time (the interval's end times interpolated as obca_plan_sweep interpolates: the track itself, across
 *   knots and turning, not a chord); a pose word of the car that is not finite: +inf.  track_clear_hist[b,step] = c (not
 *   written when c is NaN: a distance that overflowed).  c NaN: OBCA_DONE_FAILED; c < clearance and flags[b] == OBCA_RUN:
 *   OBCA_DONE_COLLISION (OBCA_DONE_GOAL stays).  A car flagged here gets variant_out[b] = 0 and every column of xref_out[b] =
 *   x0[b] (0 for a word that is not finite).  A car that did not step gets no history word and keeps its flag.
 * Then, always, for every rollout b and every j < Kt, s = K - Kt + j, t = stage 0's time:
 *   usable track  pool_A / pool_b[b,s] = obca_fleet_step's four rows of the rectangle track_size (in ego's convention) at
 *                 the pose at t, grown by margin; pool_v[b,s] = (xy(stage 1) - xy(stage 0)) / Ts[b], the chord velocity (0
 *                 for a word that is not finite), or 0 under OBCA_TRACK_PREDICT_STATIC; stage_A / stage_b[b,j,kk] = the rows
 *                 at stage kk's pose, kk = 0 .. N; stage_ok[b,j] = 1 iff predict == OBCA_TRACK_PREDICT_TRACK
 *   spare         obca_grid_pool's spare rows at `far` in the pool slot and at every stage, v = 0, stage_ok 0; also where an
 *                 interpolated pose is not finite (knot words whose difference overflows)
 * Nothing written is ever NaN.  Slots 0 .. K-Kt-1 are never touched.
 * B >= 1, 1 <= Kt <= K <= 64, 1 <= N <= 127, 1 <= L <= 4096, group >= 1 and B % group == 0, 0 <= step < max_steps <= 1024,
 * 0 <= n_sub <= 256 (0: not measured), measure 0 or 1, predict one of its three values, clearance finite (-1e300: measured,
 * never stopped), margin >= 0, far > 0 and ego finite, struct_size == sizeof(struct obca_pool_tracks), device >= 0, no pointer
 * NULL but t0 (NULL: 0 for every rollout).  Every argument is checked before the first HIP call; a refused call
 * (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
#define OBCA_TRACK_PREDICT_TRACK 0     /* the next solve reads the track's rows per stage (stage_ok = 1) */
#define OBCA_TRACK_PREDICT_VELOCITY 1  /* the rectangle now, translating at the chord velocity of the next step */
#define OBCA_TRACK_PREDICT_STATIC 2    /* the rectangle now, standing */
struct obca_pool_tracks {
    uint32_t struct_size;              /* sizeof(struct obca_pool_tracks): set by obca_pool_tracks_init() */
    uint32_t reserved_;
    int32_t B, K, Kt, N, L, group, max_steps, step, n_sub, predict;
    double clearance, margin, far;     /* obca_pool_tracks_init: -1e300 (never stops), 0 and 100 */
    double ego[4];                     /* the car's footprint; obca_pool_tracks_init: 1.7, 0.75, 1.7, 0.75 */
    /* read-only, Bt = B / group */
    const double* track_x;             /* [Bt,Kt,L,3] poses (x, y, heading) */
    const double* track_t;             /* [Bt,Kt,L] */
    const int32_t* track_len;          /* [Bt,Kt] */
    const double* track_size;          /* [Bt,Kt,4] in ego's convention */
    const double* t0;                  /* [B] or NULL */
    const double* Ts;                  /* [B] */
    const double* x_prev;              /* [B,3] the poses before the step */
    const double* x0;                  /* [B,3] the poses now */
    const int32_t* k;                  /* [B] */
    /* in and out */
    int32_t* flags;                    /* [B] */
    double* pool_A;                    /* [B,K,4,2]: slots K-Kt .. K-1 written */
    double* pool_b;                    /* [B,K,4] */
    double* pool_v;                    /* [B,K,2] */
    double* stage_A;                   /* [B,Kt,N+1,4,2] */
    double* stage_b;                   /* [B,Kt,N+1,4] */
    int32_t* stage_ok;                 /* [B,Kt] */
    int32_t* track_state;              /* [B,Kt] */
    double* track_clear_hist;          /* [B,max_steps] */
    double* xref_out;                  /* [B,3,N+1] */
    int32_t* variant_out;              /* [B] */
};   /* no typedef: the call has the descriptor's name, so C and C++ say `struct obca_pool_tracks` */

/* zero-fills *d and sets struct_size, clearance, far and ego: the one way to start filling an obca_pool_tracks */
void obca_pool_tracks_init(struct obca_pool_tracks* d);
int obca_pool_tracks(const struct obca_pool_tracks* d, int32_t measure, int32_t device, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Open-loop plans among timed tracks, on the device: a batch of plans measured against the TRACKS THEMSELVES.
 * obca_pool_tracks measures the one interval a closed loop has just driven, and obca_scene_select_staged scores a plan against
 * rows interpolated entry by entry between two stage times -- which cannot show an obstacle whose track has knots between two
 * stage times and moves in and out of the lane there.  This call samples the N intervals of a plan as obca_scene_select does
 * and puts the track's own rectangle at the track's pose at every sample's time; given obca_scene_select_staged's score it
 * folds what it measured into the running minimum that call re-ranks on (accumulate = 1), so a staged select -> solve ->
 * measure -> re-select loop takes a tracked obstacle in on the track's word.  It has no handle;
 * csrc/obca_plan_tracks_core.h holds the serial definition the kernel reproduces.
 *
 * Bt = B / group track blocks, plan b reads block b / group; track j of a block is score slot K - Kt + j.
 *   track_state   [B,Kt], written for every plan: obca_pool_tracks' rule, word for word -- 0 where track_len == 0, 1 where the
 *                 track is usable, -1 otherwise -- the plan's own time words being dt[b] finite and > 0 and t0[b] finite.  A
 *                 length outside 1 .. L is never used as an index, no knot is read before the length word and the rectangle
 *                 have passed their check, and nothing read from a track that is not in state 1 reaches an output.
 *   times         knot kk of plan b is at t0[b] + (double)kk dt[b] (one product, one sum, each rounded on its own): the word
 *                 obca_pool_tracks forms for stage kk with k = 0 and Ts = dt, so a plan's knot time and the time of the stage
 *                 row it was solved against are one word.  A caller measuring an obca_mpc4 plan passes dt = Ts * ts_opt.
 *   samples       obca_scene_select's: x0[b], where given, at knot 0's time; then for every interval s -> s + 1 the n_sub + 1
 *                 samples j = 0 .. n_sub, the car's pose interpolated as obca_plan_sweep interpolates and the time interpolated
 *                 alike between the two knot times.  A sample whose car pose is not finite is skipped.  The obstacle at a sample
 *                 is the margin-free rectangle track_size (in ego's convention) at obca_pool_tracks' pose of the track at the
 *                 sample's time: the track itself, across knots and turning.  The distance is the signed distance between the
 *                 car's footprint (ego) and obca_fleet_step's four rows of that rectangle, as obca_pool_tracks measures.
 *   measured      a plan with variant[b] != 0 and status[b] 0 or 1 (obca_scene_select's accumulate rule); a NULL variant or
 *                 status: every plan.
 *   track_clear   [B,Kt]: this call's smallest distance to track j, +inf for a slot not in state 1
 *   track_min     [B]: the smallest word of track_clear[b,:], +inf where no track is usable
 *   score         [B,K] or NULL: a measured plan gets score[b,K-Kt+j] = min(score[b,K-Kt+j], track_clear[b,j]) for every
 *                 usable j (an old word that is no number is replaced, as obca_scene_select does).  Slots 0 .. K-Kt-1 are
 *                 never touched.
 * A plan that was not measured, has no finite sample pose, or met a distance that is no number (overflow) gets NaN in
 * track_clear[b,:] and track_min[b], and its score row is untouched: the call never turns "unknown" into "safe".
 * B >= 1, 1 <= Kt <= K <= 64 (K is read only for score), 1 <= N <= 127, 1 <= L <= 4096, group >= 1 and B % group == 0,
 * 1 <= n_sub <= 256, far > 0 and ego finite, struct_size == sizeof(struct obca_plan_tracks), device >= 0, no pointer NULL but
 * t0 (NULL: 0 for every plan), x0, variant, status and score.  Every argument is checked before the first HIP call; a refused
 * call (OBCA_E_INVAL) has no side effect.  Asynchronous on hip_stream. */
struct obca_plan_tracks {
    uint32_t struct_size;              /* sizeof(struct obca_plan_tracks): set by obca_plan_tracks_init() */
    uint32_t reserved_;
    int32_t B, K, Kt, N, L, group, n_sub, reserved2_;
    double far;                        /* obca_plan_tracks_init: 100 (the spares' place; no word of this call depends on it) */
    double ego[4];                     /* the car's footprint; obca_plan_tracks_init: 1.7, 0.75, 1.7, 0.75 */
    /* read-only, Bt = B / group */
    const double* track_x;             /* [Bt,Kt,L,3] poses (x, y, heading) */
    const double* track_t;             /* [Bt,Kt,L] */
    const int32_t* track_len;          /* [Bt,Kt] */
    const double* track_size;          /* [Bt,Kt,4] in ego's convention */
    const double* t0;                  /* [B] or NULL */
    const double* dt;                  /* [B] the time between two knots of the plan */
    const double* x;                   /* [B,3,N+1] the plans */
    const double* x0;                  /* [B,3] or NULL */
    const int32_t* variant;            /* [B] or NULL */
    const int32_t* status;             /* [B] or NULL */
    /* in and out */
    double* score;                     /* [B,K] or NULL: slots K-Kt .. K-1 folded */
    /* written */
    double* track_clear;               /* [B,Kt] */
    double* track_min;                 /* [B] */
    int32_t* track_state;              /* [B,Kt] */
};   /* no typedef: the call has the descriptor's name, so C and C++ say `struct obca_plan_tracks` */

/* zero-fills *d and sets struct_size, far and ego: the one way to start filling an obca_plan_tracks */
void obca_plan_tracks_init(struct obca_plan_tracks* d);
int obca_plan_tracks(const struct obca_plan_tracks* d, int32_t device, void* hip_stream);

const char* obca_strerror(int code);
/* "obca_mpc 0.18 (gfx950)" -- the string still reads 0.18: 0.19 and 0.20 add calls and change no existing word, and callers
 * detect them by the exported symbols obca_fleet_tracks / obca_scene_select_staged and obca_pool_tracks.  Plans measured
 * against timed tracks (obca_plan_tracks) came after 0.20 in the same way: detect the call by its symbol.
 * 0.20 = obstacles on timed tracks (obca_pool_tracks);
 * 0.19 = fleet prediction by plans (obca_fleet_tracks, obca_scene_select_staged);
 * 0.18 = fleet closed loop (obca_fleet_step);
 * 0.17 = opt-in path time bound of obca_mpc4 (obca_params.time_bound, OBCA_TIME_BOUND_PATH);
 * 0.16 = closed loop over scene pools (obca_pool_loop_advance);
 * 0.15 = occupancy grids to scene pools (obca_grid_pool);
 * 0.14 = scene pools (obca_scene_select);
 * 0.13 = route-seeded open-loop planning (obca_grid_dilate_batch, obca_route_resample);
 * 0.12 = the refinement step of the two-stage open-loop planner (obca_plan_refine);
 * 0.11 = clearance repair of batched plans (obca_plan_tighten);
 * 0.10 = obca_astar_batch's code -4 (start or goal outside the grid), obca_rasterise_batch clips boxes to the map;
 * 0.9 = swept audit of batched plans (obca_plan_sweep);
 * 0.8 = opt-in swept, inflated rows of moving boxes (obca_rollouts_set_swept_rows, obca_moving_rows_batch);
 * 0.7 = opt-in collision stop (OBCA_DONE_COLLISION, obca_rollouts_set_collision_stop,
 * obca_rollouts_read_clearance) and exact sensing (obca_rollouts_set_exact_sensing); 0.6 = the answer of an exhausted start ladder is the most informative pass's (obca_params: the starts of a
 * solve), the second-order correction's scratch in LDS where it costs no occupancy; 0.5 = obca_params.struct_size (first member; obca_params_init), the dodge rung and the terminal-set screen,
 * OBCA_START_DEFAULT = the window first for obca_mpc4 too, kernel mode 5;
 * 0.2 = the start ladder (start_order / single_start / patience / retry_iter replace restart); 0.3 = second
 * level of the penalty escalation, compile-time-shape instantiations, obca_rollouts_queue_mode; 0.4 = OBCA_START_DEFAULT per variant
 * (OBCA_START_X0_FIRST moved from 0 to 3) */
const char* obca_version(void);

#ifdef __cplusplus
}
#endif
#endif
