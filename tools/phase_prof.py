"""Diagnostic: per-phase cycle shares of the step kernel (s_memtime-instrumented build; never timed)."""
import sys, os
ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT,'brax-rodent-run_amd'))
import numpy as np, torch
from rodent_amd import assets, hip, envs
from tests import util
dev=torch.device('cuda:0'); N=int(sys.argv[1]) if len(sys.argv)>1 else 2048
env=envs.get_environment('rodent', track_pos=util.synthetic_track(), num_envs=N, xml_path='rodent_optimized.xml', iterations=8, ls_iterations=8, device=dev)
state=env.reset(0)
for _ in range(30): state=env.step(state, torch.rand(N,30,device=dev)*2-1)
ps=state.pipeline_state
st=dict(qpos=ps.qpos.clone(), qvel=ps.qvel.clone(), act=ps.act.clone(), qacc_warmstart=ps.qacc_warmstart.clone())
buf=torch.zeros(N,24,dtype=torch.int64,device=dev)
b=env._batch; b.set_profile(buf)
b.pipeline_step(st, torch.rand(N,30,device=dev)*2-1, 10)
torch.cuda.synchronize()
c=buf.cpu().numpy().astype(np.float64)
names=['kinematics','com_pos','velocity_sweep','backward_sweep','mass_matrix','factor','smooth+solve','constraints','solver_init(3 ctx)','linesearch','update_constraint','update_gradient','cg_misc','euler(factor+solve)','epilogue','frame_head','ls: put_vec+jac_mul','ls: staging+sums','ls: 2 first points','ls: iterations','-','-','-','-']
NCYC=20      # slots 20 / 21 are counts, not cycles: bracketing iterations the line searches executed / left out by the repeat exit (RR_LS_REPEAT_EXIT)
tot=c[:,:NCYC].sum(1)
print(f'N={N} envs, 10 substeps; cycles per env (median over envs): total {np.median(tot):.0f}')
for i,n in enumerate(names[:NCYC]):
    print(f'  {n:26s} {np.median(c[:,i]):10.0f} cyc  {100*np.median(c[:,i]/tot):5.1f} %')
print('per-env total cycles: min %.0f  p10 %.0f  median %.0f  p90 %.0f  max %.0f  (launch time = slowest SIMD pair)' % (tot.min(), np.percentile(tot,10), np.median(tot), np.percentile(tot,90), tot.max()))
order = np.argsort(tot)
slow, mid = order[-N // 20:], order[N // 2 - N // 40:N // 2 + N // 40]
print('slowest 5 %% of the envs vs the median 5 %%, cycles per phase (the launch lasts as long as the slowest env):')
for i, n in enumerate(names[:NCYC]):
    if c[:, i].max() > 0:
        print(f'  {n:26s} slow {c[slow, i].mean():10.0f}   median {c[mid, i].mean():10.0f}   diff {c[slow, i].mean() - c[mid, i].mean():+10.0f}')
ran, left = c[:, 20], c[:, 21]
full = np.maximum(ran + left, 1)
print('bracketing iterations per env step (executed | left out by the repeat exit | share left out of what the full loop runs):')
print(f'  all envs     {ran.sum():10.0f} | {left.sum():10.0f} | {100 * left.sum() / max(ran.sum() + left.sum(), 1):5.1f} %')
print(f'  median env   {np.median(ran):10.0f} | {np.median(left):10.0f} | {100 * np.median(left / full):5.1f} %')
print(f'  median 5 %   {ran[mid].mean():10.1f} | {left[mid].mean():10.1f} | {100 * left[mid].sum() / max((ran + left)[mid].sum(), 1):5.1f} %')
print(f'  slowest 5 %  {ran[slow].mean():10.1f} | {left[slow].mean():10.1f} | {100 * left[slow].sum() / max((ran + left)[slow].sum(), 1):5.1f} %')
