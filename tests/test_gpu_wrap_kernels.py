"""The fused per-step wrapper kernels on their own (rr_wrap_episode_autoreset, rr_wrap_clip_restart, rr_wrap_clip_library,
rr_wrap_clip_sampling): the four C entries on synthetic tensors against the rule restated in plain torch
(tests/wrap_kernel_cases.py), bit for bit -- no env, no model, no step kernel.  The null-pointer combinations the entries document, the
slot clamp, both ends of `narr` and NaN rows are cases here; tests/test_wrap_kernels_cpu.py shows that the inputs contain every class of
env the rule distinguishes."""
import ctypes as C

import pytest
import torch

from rodent_amd import hip
from tests import wrap_kernel_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=X.SLOTS, ids=lambda k: f"K{k}")
def case(request):
    x = X.inputs(request.param)
    dev = {k: [t.to(DEV) for t in v] if isinstance(v, list) else (v.to(DEV) if torch.is_tensor(v) else v) for k, v in x.items()}
    return x, dev


def launch(g, level, *, narr=3, action_repeat=1.0, end_at_clip_end=True, clip=True, bank_clips=True, lengths=True, pose_fail=True,
           weights=True, outcomes=True):
    """One call of the C entry of `level` on copies of the device inputs `g`; the flags as in `wrap_kernel_cases.restate`."""
    i, K = X.LEVELS.index(level), g["K"]
    first = (g["first"] if i == 0 else g["bank"])[:narr]
    cur = [t.clone() for t in g["cur"][:narr]]
    done, steps, trunc = g["done"].clone(), torch.empty_like(g["done"]), torch.empty_like(g["done"])
    F = (C.c_void_p * narr)(*[t.data_ptr() for t in first])
    Cu = (C.c_void_p * narr)(*[t.data_ptr() for t in cur])
    W = (C.c_int32 * narr)(*X.WIDTHS[:narr])
    args = [X.N, narr, F, Cu, W, g["prev_done"].data_ptr(), g["prev_steps"].data_ptr(), done.data_ptr(), steps.data_ptr(), trunc.data_ptr(),
            X.EPISODE, float(action_repeat)]
    out = dict(done=done, steps=steps, truncation=trunc, cur=cur)
    keep = []
    if i >= 1:
        out.update(cur_frame=g["cur_frame"].clone(), slot=torch.full_like(g["slot_in"], -7))
        args += [out["cur_frame"].data_ptr(), g["bank_frames"].data_ptr(), g["slot_in"].data_ptr(), out["slot"].data_ptr(), K, X.TRACK_LEN,
                 int(end_at_clip_end)]
    if i >= 2:
        if clip:
            out["clip"] = g["clip"].clone()
        args += [out["clip"].data_ptr() if clip else None, g["bank_clips"].data_ptr() if bank_clips else None,
                 g["lengths"].data_ptr() if lengths else None]
    if i >= 3:
        if weights:
            out["draws"] = torch.full_like(g["draws"], -7)
        if outcomes:
            out["outcomes"] = g["outcomes"].clone()
        block = hip.RRClipSamplingIO(g["weights"].data_ptr() if weights else None, g["draws"].data_ptr() if weights else None,
                                     out["draws"].data_ptr() if weights else None, out["outcomes"].data_ptr() if outcomes else None, X.SEED)
        keep.append(block)
        args += [X.C, g["pose_fail"].data_ptr() if pose_fail else None, C.byref(block)]
    entry = ("rr_wrap_episode_autoreset", "rr_wrap_clip_restart", "rr_wrap_clip_library", "rr_wrap_clip_sampling")[i]
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc = getattr(hip.lib(), entry)(*args, C.c_void_p(stream))
    assert rc == 0, hip.lib().rr_last_error()
    torch.cuda.synchronize()
    return out


def check(case, level, **kw):
    x, g = case
    want, _ = X.restate(x, level, **kw)
    got = launch(g, level, **kw)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        if k == "cur":
            assert len(got[k]) == len(w)
            for a, (gt, wt) in enumerate(zip(got[k], w)):
                assert X.same_bits(gt.cpu(), wt), (level, kw, "cur", a)
        else:
            assert X.same_bits(got[k].cpu(), w), (level, kw, k, got[k].tolist(), w.tolist())
    return got, want


@pytest.mark.parametrize("level", X.LEVELS)
def test_each_entry_follows_the_rule(case, level):                                       # a
    check(case, level)


@pytest.mark.parametrize("action_repeat", [1.0, 2.0])
def test_plain_entry_action_repeat(case, action_repeat):                                 # b
    check(case, "plain", action_repeat=action_repeat)


@pytest.mark.parametrize("narr", [0, 12])
def test_plain_entry_at_both_ends_of_narr(case, narr):                                   # c, d: bookkeeping only; RR_WRAP_MAX arrays
    got, _ = check(case, "plain", narr=narr)
    assert len(got["cur"]) == narr


@pytest.mark.parametrize("clip,bank_clips,lengths", [(False, False, True), (True, True, False), (True, True, True)],
                         ids=["lengths_only_clip_null", "bank_clips_only", "both"])
def test_library_entry_null_pointer_combinations(case, clip, bank_clips, lengths):      # e, f, g
    _, want = check(case, "library", clip=clip, bank_clips=bank_clips, lengths=lengths)
    assert ("clip" in want) == clip


@pytest.mark.parametrize("weights,outcomes,pose_fail", [(False, True, True), (True, False, True), (True, True, True), (True, True, False)],
                         ids=["outcomes_only", "weights_only", "both", "both_without_pose_fail"])
def test_sampling_entry_null_pointer_combinations(case, weights, outcomes, pose_fail):  # h, i, j
    _, want = check(case, "sampling", weights=weights, outcomes=outcomes, pose_fail=pose_fail)
    assert ("draws" in want) == weights and ("outcomes" in want) == outcomes


def test_sampling_entry_counts_without_the_library(case):                                # h: counting alone, clip ids only
    check(case, "sampling", weights=False, bank_clips=False, lengths=False)


@pytest.mark.parametrize("level", X.LEVELS[1:])
@pytest.mark.parametrize("end_at_clip_end", [False, True])
def test_end_at_clip_end_on_the_same_inputs(case, level, end_at_clip_end):               # k
    check(case, level, end_at_clip_end=end_at_clip_end)


@pytest.mark.parametrize("level", X.LEVELS)
def test_nan_rows_are_replaced_where_done_and_kept_where_not(case, level):               # l, m
    got, _ = check(case, level)
    x, _ = case
    bits = lambda t: t.cpu().contiguous().view(torch.int32)
    for a, col in ((0, 0), (1, 2), (2, 257), (2, 299)):
        assert bits(x["cur"][a])[X.LIVE_ENV, col] == X.NAN_BITS and bits(got["cur"][a])[X.LIVE_ENV, col] == X.NAN_BITS
        assert bits(x["cur"][a])[X.DONE_ENV, col] == X.NAN_BITS and not torch.isnan(got["cur"][a][X.DONE_ENV, col])
    assert got["done"][X.DONE_ENV] == 1 and got["done"][X.LIVE_ENV] == 0
    assert bits(got["cur"][1])[X.DONE_ENV, 0] == X.NAN_BITS          # the stored NaN came back, payload included


def test_the_bindings_call_the_narrowest_entry(case, monkeypatch):
    """`hip.wrap_episode_autoreset` and `hip.wrap_clip` on the same inputs: the entry each call reaches, and the entries' results."""
    x, g = case
    called = []
    for name in ("rr_wrap_episode_autoreset", "rr_wrap_clip_restart", "rr_wrap_clip_library", "rr_wrap_clip_sampling"):
        def spy(*a, _real=getattr(hip.lib(), name), _name=name):
            called.append(_name)
            return _real(*a)
        monkeypatch.setattr(hip.lib(), name, spy)

    def run(level, **kw):
        i = X.LEVELS.index(level)
        cur = [t.clone() for t in g["cur"][:3]]
        out = dict(done=g["done"].clone(), steps=torch.empty_like(g["done"]), truncation=torch.empty_like(g["done"]), cur=cur)
        common = (cur, g["prev_done"], g["prev_steps"], out["done"], out["steps"], out["truncation"], X.EPISODE, 1.0)
        if i == 0:
            hip.wrap_episode_autoreset(g["first"][:3], *common)
        else:
            out.update(cur_frame=g["cur_frame"].clone(), slot=torch.empty_like(g["slot_in"]))
            for k in kw:
                if k in ("clip", "outcomes"):      # finished / added to in place: a copy per call, whatever placeholder the caller gave
                    out[k] = g[k].clone()
                    kw[k] = out[k]
            if "draws_in" in kw:
                out["draws"] = kw["draws_out"] = torch.empty_like(g["draws"])
            hip.wrap_clip(g["bank"][:3], *common, out["cur_frame"], g["bank_frames"], g["slot_in"], out["slot"], X.TRACK_LEN, True, **kw)
        torch.cuda.synchronize()
        want, _ = X.restate(x, level)
        assert set(out) == set(want)
        assert all(X.same_bits(a.cpu(), b) for k in want for a, b in (zip(out[k], want[k]) if k == "cur" else [(out[k], want[k])])), level

    lib_kw = dict(clip=None, bank_clips=g["bank_clips"], lengths=g["lengths"])
    run("plain")
    run("restart")
    run("library", **lib_kw)
    run("sampling", num_clips=X.C, pose_fail=g["pose_fail"], weights=g["weights"], draws_in=g["draws"], outcomes=None, seed=X.SEED, **lib_kw)
    assert called == ["rr_wrap_episode_autoreset", "rr_wrap_clip_restart", "rr_wrap_clip_library", "rr_wrap_clip_sampling"]
