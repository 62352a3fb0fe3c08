"""Multi-clip tracking on the GPU: a batch whose envs follow different clips of a [C, T, 3] track (`rr_env_io.clip`) against plain
single-clip batches of the same build -- bit for bit, envs being independent and the kernel bit-reproducible -- and against the
reward / observation formulas.

Fixture: N = 12 envs, C = 3 clips, env e on clip e % 3 (explicit ids); n_frames = 2, solver iterations 4 / 4.  Two track sets: T = 104
(start frames are 0 .. 99: within five steps the two envs that start at frame 99 run past the clip's end, the others do not) and T = 3
(every access clamps; a clamp on the GLOBAL row index would hand clip 0 the rows of clip 1).  The clips lie 10 cm apart at every frame
(the reset noise alone puts an env up to 1.7 cm from its own), so a wrong clip changes pos_reward = exp(-100 |dx|) by far more than a
factor of e.  Models: rodent_optimized (fixed dimensions), rodent_0
(generic), rodent_cpu (candidate pairs)."""
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from tests import randomisation_sets as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, C, STEPS = 12, 3, 5
SEED = 78            # start frames [42, 99, 35, 32, 33, 99, 10, 46, 47, 47, 19, 51]
IDS = np.arange(N) % C
MODELS = ["rodent_optimized", "rodent_0", "rodent_cpu"]
EPS = 2.0 ** -24


def _tracks(T):
    t = np.arange(T, dtype=np.float64)
    return np.stack([np.stack([0.004 * t, np.full(T, 0.1 * c), np.full(T, 0.0681 + 0.002 * c)], axis=1) for c in range(C)])


def _make(model, track, n, **kw):
    from rodent_amd import envs
    if model == "rodent_cpu":                    # qpos[2] is a hinge angle there (tests/test_gpu_unroll_self_collision.py)
        kw.setdefault("healthy_z_range", (-0.3, 0.3))
    return envs.get_environment("rodent", track_pos=track, num_envs=n, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                device=DEV, **kw)


def _keys():
    return jax_random.split(jax_random.PRNGKey(SEED), N)


def _reset(env, keys, clip):
    return env.reset(keys) if clip is None else env.reset(keys, clip=clip)


def _leaves(state):
    from rodent_amd.envs import graphed
    return graphed.tree_leaves(state.replace(info={k: v for k, v in state.info.items() if k != "clip"}))


def _assert_same(got, want, rows=None, what=""):
    """Every leaf of the two states (info['clip'] aside) equal bit for bit; `rows`: the envs of `got` that `want` holds."""
    la, lb = _leaves(got), _leaves(want)
    assert len(la) == len(lb) > 10
    for i, (x, y) in enumerate(zip(la, lb)):
        x = x if rows is None else x[rows]
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i, int((x != y).sum()))


def _assert_clip_kept(state, ids=IDS):
    assert state.info["clip"].dtype == torch.int32 and state.info["clip"].cpu().tolist() == list(ids)


def _actor(env, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return acting.actor_params(net, norm, dist.min_std)


def _draws(env, T, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    A = env.action_size
    return torch.rand(T, N, A, device=DEV, generator=gen) * 2 - 1, torch.randn(T, N, A, device=DEV, generator=gen)


def _steps(env, keys, acts, clip=None):
    """The reset state and the state after each plain `step`."""
    out = [_reset(env, keys, clip)]
    for t in range(acts.shape[0]):
        out.append(env.step(out[-1], acts[t]))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [104, 3])
@pytest.mark.parametrize("model", MODELS)
def test_mixed_batch_equals_single_clip_batches(model, T):
    """Reset and five steps of the mixed batch against a plain `Rodent(track_pos=tracks[c], num_envs=4)` per clip on the keys and actions
    of its envs: qpos, qvel, act, warm start, obs, reward, done, metrics and cur_frame, every leaf of the state."""
    tracks, keys = _tracks(T), _keys()
    mixed = _make(model, tracks, N)
    assert mixed.num_clips == C
    acts, _ = _draws(mixed, STEPS, 1)
    got = _steps(mixed, keys, acts, IDS)
    for s in got:
        _assert_clip_kept(s)
    frames = got[-1].info["cur_frame"].cpu().numpy()
    if T == 104:
        assert (frames + 1 > T - 1).sum() >= 2 and (frames + 1 < T - 1).sum() >= 6         # past the end / inside the clip
    for c in range(C):
        rows = torch.arange(c, N, C, device=DEV)
        plain = _make(model, tracks[c], N // C)
        assert plain.num_clips == 1
        want = _steps(plain, keys[c::C], acts[:, rows].contiguous())
        for t, (g, w) in enumerate(zip(got, want)):
            assert "clip" not in w.info
            _assert_same(g, w, rows, what=(model, T, c, t))
    assert float(got[-1].metrics["pos_reward"].max()) > 0 and torch.isfinite(got[-1].obs).all()


def _traj(buf):
    return dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])


BUF = ("obs", "raw_action", "log_prob", "reward", "discount", "truncation")


def _wrapped_forms(env, keys, acts, noise, actor, clip=None, evaluation=True):
    """The multi-step forms under Episode(3) + AutoReset on one env: `unroll`; `unroll_policy` into trajectory buffers; and, with
    `evaluation`, `unroll_eval` wrapped (EvalWrapper.unroll_policy) and raw, each with qpos_out (the wrapped one with eval_metrics)."""
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    T, n = acts.shape[0], env.num_envs
    wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
    out = dict(unroll=wenv.unroll(_reset(wenv, keys, clip), acts))
    buf = acting.UnrollBuffer(1, n, T, env.observation_size, env.action_size, torch.device(DEV))
    out["policy"], out["policy_actions"] = wenv.unroll_policy(_reset(wenv, keys, clip), actor, noise, _traj(buf))
    out["buf"] = buf
    if evaluation:
        ew = wrappers.EvalWrapper(wenv)
        assert ew.unroll_supported()
        out["eval_qpos"] = torch.empty(T + 1, n, env.sys.nq, device=DEV)
        out["eval"] = ew.unroll_policy(_reset(ew, keys, clip), actor, noise, T, qpos_out=out["eval_qpos"])
        out["raw_qpos"] = torch.empty(T + 1, n, env.sys.nq, device=DEV)
        out["raw"] = env.unroll_eval(_reset(env, keys, clip), T, actor, noise, qpos_out=out["raw_qpos"])
    torch.cuda.synchronize()
    return out


def _assert_forms_same(got, want, rows, what):
    for k, w in want.items():
        g = got[k]
        if k == "buf":
            for name in BUF:
                assert torch.equal(getattr(g, name)[:, rows], getattr(w, name)), (what, name)
        elif torch.is_tensor(w):
            assert torch.equal(g[:, rows], w), (what, k)
        else:
            _assert_same(g, w, rows, what=(what, k))


@pytest.mark.parametrize("T", [104, 3])
@pytest.mark.parametrize("model", MODELS)
def test_wrapped_forms_equal_single_clip_batches(model, T):
    """Seven steps with episodes of three, so restores happen inside every launch: each form of the mixed batch equals the same form of
    the per-clip plain batches, and info['clip'] comes back unchanged (a restore leaves it alone, as it leaves cur_frame)."""
    U = 7
    tracks, keys = _tracks(T), _keys()
    mixed = _make(model, tracks, N)
    assert mixed._batch.unroll_supported(False) and mixed._batch.unroll_supported(True) and mixed.eval_supported()
    actor = _actor(mixed, 7)
    acts, noise = _draws(mixed, U, 2)
    got = _wrapped_forms(mixed, keys, acts, noise, actor, IDS)
    for k in ("unroll", "policy", "eval", "raw"):
        _assert_clip_kept(got[k])
    assert float(got["unroll"].info["steps"].max()) <= 3 and bool((got["buf"].discount == 0).any())        # episodes ended: restores ran
    assert 0 < float(got["eval"].info["eval_metrics"]["episode_steps"].max()) <= 3
    for c in range(C):
        rows = torch.arange(c, N, C, device=DEV)
        plain = _make(model, tracks[c], N // C)
        want = _wrapped_forms(plain, keys[c::C], acts[:, rows].contiguous(), noise[:, rows].contiguous(), actor)
        _assert_forms_same(got, want, rows, (model, T, c))


@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_0"])
def test_per_env_parameters_with_clips(model):
    """Every env carrying the model's own rows (the rr_rand_kernel instances) plus clips equals plain plus clips: wrapped single steps,
    the multi-step launch and the launch with the actor inside.  (A batch with per-env parameters has no evaluation instance.)"""
    from rodent_amd.envs import wrappers
    from rodent_amd.ktables import env_param_tables
    U = 7
    tracks, keys = _tracks(104), _keys()
    plain, rand = _make(model, tracks, N), _make(model, tracks, N)
    m = rand.sys.tables
    ident = {k: np.repeat(v[None], N, axis=0) for k, v in rs.base_fields(m).items()}
    rand.set_env_params(*(torch.from_numpy(a).to(DEV) for a in env_param_tables(m, ident)))
    assert rand.env_params() is not None and plain.env_params() is None
    actor = _actor(plain, 9)
    acts, noise = _draws(plain, U, 3)
    res = []
    for env in (plain, rand):
        wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
        s = wenv.reset(keys, clip=IDS)
        for t in range(U):
            s = wenv.step(s, acts[t])
        forms = _wrapped_forms(env, keys, acts, noise, actor, IDS, evaluation=False)
        forms["steps"] = s
        res.append(forms)
    rows = torch.arange(N, device=DEV)
    _assert_forms_same(res[1], res[0], rows, model)
    _assert_clip_kept(res[1]["steps"])


@pytest.mark.parametrize("model,T", [("rodent_optimized", 104), ("rodent_optimized", 3), ("rodent_0", 104)])
def test_against_the_formula(model, T):
    """From the returned states of an env with `pipeline_outputs=True`, float64 arithmetic on the float32 values the kernel read:

        metrics pos_reward = exp(-100 |qpos[:3] - tracks[clip][clamp(old_frame)]|)
        obs[-3:]           = xmat[1] @ (tracks[clip][clamp(new_frame + 1)] - qpos[:3])

    Tolerances (eps = 2^-24, the float32 unit roundoff).  pos_reward: the three differences, three squares, two sums and the square root
    leave |dx| with a relative error below 4 eps; the product with -100 adds one, so the argument x = 100 |dx| of expf carries at most
    5 eps x, which the exponential turns into a RELATIVE error of the result; expf itself is good to 2 ulp = 4 eps.  Bound:
    (5 x + 4) eps * pos_reward, doubled for the slack of a first-order count.  obs[-3:]: each difference v_k carries eps |v_k|, each
    element of xmat (|m| <= 1, formed from the unit quaternion by a handful of products and sums) an absolute error of at most 8 eps,
    each product and each of the two sums another eps: |error| <= 12 eps * sum |v_k|, doubled likewise.  A wrong clip moves the target
    by 10 cm: pos_reward by more than a factor of e, the observation by |10 cm| rotated -- four orders of magnitude above either bound."""
    tracks, keys = _tracks(T), _keys()
    env = _make(model, tracks, N, pipeline_outputs=True)
    acts, _ = _draws(env, STEPS, 4)
    states = _steps(env, keys, acts, IDS)
    tr32 = tracks.astype(np.float32).astype(np.float64)
    at = lambda frame: tr32[IDS, np.clip(frame, 0, T - 1)]
    worst = [0.0, 0.0]
    for t in range(STEPS + 1):
        s = states[t]
        qpos3 = s.pipeline_state.qpos[:, :3].cpu().numpy().astype(np.float64)
        new_frame = s.info["cur_frame"].cpu().numpy()
        xmat1 = s.pipeline_state.xmat[:, 1].cpu().numpy().astype(np.float64).reshape(N, 3, 3)
        v = at(new_frame + 1) - qpos3
        want = np.einsum("nij,nj->ni", xmat1, v)
        got = s.obs[:, -3:].cpu().numpy().astype(np.float64)
        bound = 24 * EPS * np.abs(v).sum(1, keepdims=True)
        worst[0] = max(worst[0], float((np.abs(got - want) / bound).max()))
        assert (np.abs(got - want) <= bound).all(), (t, np.abs(got - want).max(), bound.min())
        other = np.einsum("nij,nj->ni", xmat1, tr32[(IDS + 1) % C, np.clip(new_frame + 1, 0, T - 1)] - qpos3)
        assert (np.abs(other - want).max(1) > 1e4 * bound[:, 0]).all()                      # the neighbouring clip is far outside
        if t == 0:
            continue
        old_frame = states[t - 1].info["cur_frame"].cpu().numpy()
        assert np.array_equal(new_frame, old_frame + 1)
        x = 100.0 * np.linalg.norm(qpos3 - at(old_frame), axis=1)
        want_r, got_r = np.exp(-x), s.metrics["pos_reward"].cpu().numpy().astype(np.float64)
        bound_r = 2 * (5 * x + 4) * EPS * want_r
        worst[1] = max(worst[1], float((np.abs(got_r - want_r) / bound_r).max()))
        assert (np.abs(got_r - want_r) <= bound_r).all(), (t, np.abs(got_r - want_r).max(), bound_r.min())
        other_r = np.exp(-100.0 * np.linalg.norm(qpos3 - tr32[(IDS + 1) % C, np.clip(old_frame, 0, T - 1)], axis=1))
        assert (np.abs(np.log(other_r / want_r)) > 1).all()                                 # a wrong clip: more than a factor of e
    print(f"{model} T={T}: largest |error| / bound: obs[-3:] {worst[0]:.3f}, pos_reward {worst[1]:.3f}")


@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_0"])
def test_one_clip_and_two_dimensions(model):
    """[1, T, 3] equals [T, 3] bit for bit (drawn id and explicit id alike); the 2-D state has no 'clip' key and refuses one."""
    tracks, keys = _tracks(104), _keys()
    flat, one = _make(model, tracks[1], N), _make(model, tracks[1:2], N)
    assert flat.num_clips == 1 and one.num_clips == 1 and one.with_num_envs(4)._track_pos.shape == (1, 104, 3)
    acts, _ = _draws(flat, STEPS, 5)
    want = _steps(flat, keys, acts)
    for clip in (None, 0):
        got = _steps(one, keys, acts, clip)
        for g, w in zip(got, want):
            assert "clip" not in w.info and g.info["clip"].cpu().tolist() == [0] * N
            _assert_same(g, w)
    with pytest.raises(ValueError, match="single"):
        flat.reset(keys, clip=0)
    with pytest.raises(ValueError, match="clip ids must lie"):
        one.reset(keys, clip=1)


def test_ppo_train_on_two_clips(monkeypatch):
    """8 envs on two clips, one training step through the one-launch rollout, evaluations on 6 envs: finite losses, the existing eval
    keys, and eval/episode_reward_clip{c} for exactly the clips the eval envs drew, consistent with the overall mean."""
    from rodent_amd import envs
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    tracks = _tracks(104)[:2]
    env = _make("rodent_optimized", tracks, 8)
    eval_env = env.with_num_envs(6)
    assert eval_env.num_clips == 2
    calls, last, evals, log = {"fused": 0}, {}, [], []
    real_fused, real_reset, real_eval = acting.generate_unrolls_fused, envs.Rodent.reset, acting.Evaluator.run_evaluation
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])

    def reset(self, rng, clip=None):
        st = real_reset(self, rng, clip)
        if self is eval_env:
            last["ids"] = st.info["clip"].cpu().numpy().copy()
        return st

    def run_evaluation(self, *a, **k):
        m = real_eval(self, *a, **k)
        evals.append((m, last.pop("ids")))           # the ids of THIS evaluation's reset
        return m
    monkeypatch.setattr(envs.Rodent, "reset", reset)
    monkeypatch.setattr(acting.Evaluator, "run_evaluation", run_evaluation)
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=8, batch_size=8, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=2, num_eval_envs=6, eval_env=eval_env, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m))
    assert calls["fused"] == 1
    assert len(evals) >= 2 and math.isfinite(float(log[-1]["training/total_loss"]))
    for m, ids in evals:
        want = {f"eval/episode_reward_clip{c}" for c in np.unique(ids)}
        assert {k for k in m if k.startswith("eval/episode_reward_clip")} == want and 1 <= len(want) <= 2
        for k in ("eval/episode_reward", "eval/episode_pos_reward", "eval/episode_reward_quadctrl", "eval/episode_reward_alive",
                  "eval/avg_episode_length", "eval/epoch_eval_time", "eval/sps", "eval/walltime"):
            assert k in m and math.isfinite(float(m[k])), k
        # the per-clip means, weighted by their envs, give the overall mean: float32 means of at most 6 values, bound 8 eps each
        mean = sum(float(m[f"eval/episode_reward_clip{c}"]) * int((ids == c).sum()) for c in np.unique(ids)) / len(ids)
        scale = max(abs(float(m[k])) for k in list(want) + ["eval/episode_reward"])
        assert abs(mean - float(m["eval/episode_reward"])) <= 32 * EPS * max(scale, 1.0)
