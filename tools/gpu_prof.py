"""dev tool: per-phase shader-clock shares of the solver (library built by tools/build_variant.sh prof -DOBCA_PROFILE):
python tools/gpu_prof.py B c2|c3|c3free N     (OBCA_LIB=<file name inside the package>: another instrumented build, e.g. the parent's)"""
import os, sys, ctypes, numpy as np, torch
sys.path.insert(0, '.')
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib, scenarios as sc
_lib.LIB_PATH = os.path.join(_lib.HERE, os.environ.get('OBCA_LIB', 'libobca_mpc_prof.so'))
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import BatchSolver, SolverParams
B=int(sys.argv[1]) if len(sys.argv)>1 else 768
N=int(sys.argv[3]) if len(sys.argv)>3 else 5
kind=sys.argv[2] if len(sys.argv)>2 else 'c2'
b=sc.make_batch_c3(B,N,gated=True) if kind=='c3' else sc.make_batch_c3(B,N,gated=False) if kind=='c3free' else sc.make_batch(B,N)
s=BatchSolver(N,b['m'],B)
prof=torch.zeros(B,20,dtype=torch.float64,device='cuda')
s.lib.obca_set_profile_buffer(s._h, ctypes.c_void_p(prof.data_ptr()))
for _ in range(2):
    out=s.solve(b['variant'],b['x0'],b['u0'],b['xref'],b['A'],b['b'],b['Ts'],b['term'],SolverParams())
torch.cuda.synchronize()
p=prof.cpu().numpy(); it=out.iters.cpu().numpy(); nf=out.info[:,3].cpu().numpy()
# Slots 18 / 19 mean different things in different builds.  One-wavefront kernels (shapes of at most 384 rows, include/obca_mpc.h): clocks of
# rowsteps' slot loop and staging loop.  Four-wavefront kernels: counts of two-sided sweeps, or, in a -DOBCA_TWO_SIDED_CHECK build, step
# differences -- the two branches below, which therefore only apply above 384 rows (as before the clocks existed; a shape above 384 rows that
# mode "global1" runs on one wavefront is still read their way).  Rows from the handle: the dual vector is the rows plus two per (stage, obstacle).
rows = int(s.lib.obca_dual_size(ctypes.byref(s._dims))) - 2*(N+1)*len(b['m'])
onewave = rows <= 384
if onewave:
    pass                                                        # clocks: printed with the others below
elif p[:,19].max() > 0 and p[:,18].max() <= p[:,19].max():     # four-wavefront kernels: share of the solves whose sweep ran two-sided
    print('two-sided sweeps: %.3f of the solves (%.3f more with E^-1 in (1e6, 4e6])' % (p[:,18].sum()/p[:,19].sum(), p[:,10].sum()/p[:,19].sum()))
    p[:,18:] = 0; p[:,10] = 0
elif p[:,18].max() > 0:     # library built with -DOBCA_TWO_SIDED_CHECK: slots 18 / 19 hold step differences, not clocks
    print('two-sided vs one-sided sweep, same data: max rel. difference of the step %.2e (median of per-instance maxima %.2e), of the elastic multiplier steps %.2e (median %.2e)'
          % (p[:,18].max()/1e18, np.median(p[:,18])/1e18, p[:,19].max()/1e18, np.median(p[:,19])/1e18))
    p[:,18:] = 0
if os.environ.get('OBCA_MATH_COUNT'):     # library built with -DOBCA_PROFILE -DOBCA_MATH_COUNT: slots 12 / 13 / 14 hold counts, not the sweep's first three clocks
    tr, re_, pw = (p[:,i].sum()/it.sum() for i in (12, 13, 14))
    print('per iteration: line-search trials %.4f, evaluations of phi(x_k) in rowsteps %.4f, iterations forming the two powers %.4f -> dlog calls %.3f (one per row slot, %d slots), dsincos calls %.3f, dpow calls %.3f'
          % (tr, re_, pw, -(-rows//64)*(tr+re_), -(-rows//64), tr, 2*pw))
    p[:,12:15] = 0
names=["grad+err","mu","rowE+gatherB","asm_stages","local","riccati","rowsteps","linesearch","accept","reeval","prologue","loop","r:FG+term","r:phaseA","r:phaseB","r:stage0","r:forward","r:recover","rs:slotloop","rs:staging"]      # one-wavefront kernels: rowsteps' rolled staging loop (row_jdx) and unrolled slot loop; "rowsteps" is the rest of that phase
tot=p[:,:12].sum(1)+(p[:,18]+p[:,19] if onewave else 0)
print('mean iters %.1f nfact %.1f total cycles/solve %.3e'%(it.mean(), nf.mean(), tot.mean()))
for i,n in enumerate(names):
    print('%-14s %6.2f%%  cycles/iter %9.0f'%(n, 100*p[:,i].sum()/tot.sum(), p[:,i].sum()/it.sum()))
st=out.status.cpu().numpy(); print('status counts', {int(k):int((st==k).sum()) for k in np.unique(st)})
