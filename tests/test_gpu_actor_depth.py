"""GPU: the in-kernel actor (`rr_actor_step` of csrc/rr_kernel.h, inside rr_env_unroll_policy and rr_env_unroll_eval) at the depths
other than the default four hidden layers: 1, 2 and 3 (which `acting.actor_shape_supported` routes to it in `ppo.train`) and 5 (which
the kernel evaluates and `acting.actor_params` builds, but `ppo.train` does not route).  Per depth the checks and bounds of
tests/test_gpu_ppo.py::test_one_launch_unroll_with_the_actor_inside -- replay through the per-step path, the two-launch actor on the
recorded observations -- plus the float64 policy; the evaluation form by the checks of tests/test_gpu_eval_unroll.py; the two-pass head
(38 actuators) at the two extremes; and the refusal of a sixth hidden layer.

`_assert_matches_replay` (tests/test_gpu_eval_unroll.py) and `_policy64`, `Z_BAND` (tests/test_gpu_unroll_self_collision.py) are those files'
own helpers, imported so that the bounds here are theirs and not copies of them (as tests/test_gpu_policy_head.py imports from
tests/test_gpu_ppo_loss.py); a rename there has to be followed here."""
import pytest
import torch

from tests import mlp_shapes as S, util
from tests.test_gpu_eval_unroll import _assert_matches_replay
from tests.test_gpu_unroll_self_collision import Z_BAND, _policy64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP_SUMS = ("pos_reward", "reward")


def _env(model, N, episode_length, iters, z_range, key):
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path=model, iterations=iters, ls_iterations=iters,
                               device=DEV, healthy_z_range=z_range)
    wenv = wrappers.wrap(env, episode_length=episode_length, action_repeat=1)
    return env, wenv, jax_random.split(jax_random.PRNGKey(key), N)


def _policy(env, depth, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, policy_hidden_layer_sizes=(32,) * depth, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return net, dist, norm, acting.actor_params(net, norm, dist.min_std)


def _unroll_and_check(model, depth, N, T, episode_length, iters, z_range):
    from rodent_amd import hip
    from rodent_amd.training import acting, fused_mlp
    env, wenv, keys = _env(model, N, episode_length, iters, z_range, 2)
    st0 = wenv.reset(keys)
    net, dist, norm, actor = _policy(env, depth, 10 + depth)
    assert len(actor["hidden_wt"]) == depth - 1 and acting.actor_shape_supported(net, env.action_size) == (depth <= 4)
    A = env.action_size
    buf = acting.UnrollBuffer(1, N, T, env.observation_size, A, torch.device(DEV))
    noise = torch.randn(T, N, A, device=DEV)
    traj = dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])
    got, actions = wenv.unroll_policy(st0, actor, noise, traj)
    torch.cuda.synchronize()
    assert torch.isfinite(buf.obs[0]).all() and torch.isfinite(buf.log_prob[0]).all()
    # (1) physics + wrappers: replay the recorded actions step by step
    _, wenv2, _ = _env(model, N, episode_length, iters, z_range, 2)
    st = wenv2.reset(keys)
    for t in range(T):
        assert torch.equal(buf.obs[0, :, t], st.obs), t
        st = wenv2.step(st, actions[t])
        assert (buf.reward[0, :, t] - st.reward).abs().max() <= 2.5e-7 and torch.equal(buf.discount[0, :, t], 1 - st.done), t
        assert torch.equal(buf.truncation[0, :, t], st.info["truncation"]), t
    assert torch.equal(buf.obs[0, :, T], st.obs) and torch.equal(got.obs, st.obs) and torch.equal(got.pipeline_state.qpos, st.pipeline_state.qpos)
    assert float(buf.truncation[0].sum()) > 0                          # an episode ended inside the launch: the reset path ran
    # (2) the two-launch actor on the recorded observations, same noise
    obs_t = buf.obs[0, :, :T].transpose(0, 1).reshape(T * N, -1).contiguous()
    flat_noise = noise.reshape(T * N, -1).contiguous()
    act, raw, lp, _ = hip.policy_act(obs_t, norm.mean, norm.std, fused_mlp.net_params(net), flat_noise, dist.min_std)
    raw_k = buf.raw_action[0].transpose(0, 1).reshape(T * N, -1)
    lp_k = buf.log_prob[0].transpose(0, 1).reshape(-1)
    act_k = actions.reshape(T * N, -1)
    assert (raw_k - raw).abs().max() <= 2e-5 * max(1.0, float(raw.abs().max()))
    assert (act_k - act).abs().max() <= 2e-5
    assert (lp_k - lp).abs().max() <= 2e-3
    # (3) the float64 policy, same bounds
    raw64, act64, lp64 = _policy64(net, norm, obs_t, flat_noise, dist.min_std)
    e_raw = float((raw_k.double() - raw64).abs().max()) / max(1.0, float(raw64.abs().max()))
    e_act, e_lp = float((act_k.double() - act64).abs().max()), float((lp_k.double() - lp64).abs().max())
    print(f"{model} depth {depth}: actor vs float64: raw {e_raw:.3g} (rel), action {e_act:.3g}, log-prob {e_lp:.3g}")
    S.record(f"in-kernel actor {model} depth={depth}", "raw vs float64 (relative)", e_raw, None)
    S.record(f"in-kernel actor {model} depth={depth}", "action vs float64", e_act, None)
    S.record(f"in-kernel actor {model} depth={depth}", "log-prob vs float64", e_lp, None)
    assert e_raw <= 2e-5 and e_act <= 2e-5 and e_lp <= 2e-3


@pytest.mark.parametrize("depth", S.ACTOR_DEPTHS)
def test_one_launch_unroll_at_other_depths(depth):
    """rodent_optimized.xml, 8 envs, 4 steps, episodes of 3 steps (a reset inside the launch)."""
    _unroll_and_check("rodent_optimized.xml", depth, 8, 4, 3, 8, (0.045, 0.5))


@pytest.mark.parametrize("depth", [1, 5])
def test_one_launch_unroll_at_other_depths_38_actuators(depth):
    """rodent_cpu.xml (76 logits: the head's two passes), 8 envs, 3 steps, episodes of 2 steps."""
    _unroll_and_check("rodent_cpu.xml", depth, 8, 3, 2, 6, Z_BAND)


@pytest.mark.parametrize("depth", [1, 5])
@pytest.mark.parametrize("sampled", [False, True])
def test_eval_unroll_at_other_depths(depth, sampled):
    """rr_env_unroll_eval, deterministic and sampled: the launch leaves what EvalWrapper.step leaves on the recorded actions
    (tests/test_gpu_eval_unroll.py `_assert_matches_replay`), and every recorded action is `hip.policy_act`'s on the observation the
    replay holds at that step, to the 2e-5 that file holds the in-kernel actor's actions to."""
    from rodent_amd import hip
    from rodent_amd.envs import wrappers
    from rodent_amd.training import fused_mlp
    N, EP, T = 8, 3, 4
    env, wenv, keys = _env("rodent_optimized.xml", N, EP, 8, (0.03, 0.5), 2)
    ew = wrappers.EvalWrapper(wenv)
    st0 = ew.reset(keys)
    net, dist, norm, actor = _policy(env, depth, 20 + depth)
    assert ew.unroll_supported() and env.eval_supported()
    noise = torch.randn(T, N, env.action_size, device=DEV) if sampled else None
    actions = torch.empty(T, N, env.action_size, device=DEV)
    got = ew.unroll_policy(st0, actor, noise, T, actions_out=actions)
    torch.cuda.synchronize()
    assert torch.isfinite(actions).all() and float(actions.abs().max()) <= 1
    _, wenv2, _ = _env("rodent_optimized.xml", N, EP, 8, (0.03, 0.5), 2)
    ew2 = wrappers.EvalWrapper(wenv2)
    st, partial, act_err = ew2.reset(keys), 0.0, 0.0
    for t in range(T):
        a = hip.policy_act(st.obs.contiguous(), norm.mean, norm.std, fused_mlp.net_params(net), noise[t].contiguous() if sampled else None, dist.min_std)[0]
        act_err = max(act_err, float((a - actions[t]).abs().max()))
        st = ew2.step(st, actions[t])
        em = st.info["eval_metrics"]["episode_metrics"]
        partial = max(partial, *(float(em[k].abs().max()) for k in ULP_SUMS))
    print(f"depth {depth} sampled {sampled}: largest |policy_act(obs) - action| = {act_err:.3g}")
    S.record(f"eval unroll depth={depth} sampled={int(sampled)}", "action vs policy_act", act_err, None)
    assert act_err <= 2e-5
    _assert_matches_replay(got, st, T, partial)


def test_a_sixth_hidden_layer_is_refused():
    """Six hidden layers are refused before anything is launched: the trajectory buffers keep their fill.  What raises today is
    `hip.Batch._actor_io`, and only by the size of its ctypes array: `rr_actor_io` has four hidden-weight slots, and five initialisers
    for `(c_void_p * 4)` are an IndexError.  Neither `acting.actor_params` nor `_actor_io` checks the depth itself, and the library's own
    limit (`actor_limit`, 1 .. 5 hidden layers, RuntimeError through `_check`) is never reached.  An explicit depth check in either Python
    function (a ValueError) would be the intended replacement, so all three exception types count as the refusal."""
    from rodent_amd.training import acting
    N, T = 8, 2
    env, wenv, keys = _env("rodent_optimized.xml", N, 3, 8, (0.045, 0.5), 2)
    st0 = wenv.reset(keys)
    buf = acting.UnrollBuffer(1, N, T, env.observation_size, env.action_size, torch.device(DEV))
    for t in (buf.obs, buf.raw_action, buf.log_prob, buf.reward, buf.discount, buf.truncation):
        t.fill_(-7.0)
    traj = dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])
    with pytest.raises((ValueError, IndexError, RuntimeError)):
        _, _, _, actor = _policy(env, S.ACTOR_REFUSED_DEPTH, 1)
        wenv.unroll_policy(st0, actor, torch.randn(T, N, env.action_size, device=DEV), traj)
    torch.cuda.synchronize()
    for t in (buf.obs, buf.raw_action, buf.log_prob, buf.reward, buf.discount, buf.truncation):
        assert bool((t == -7.0).all())
