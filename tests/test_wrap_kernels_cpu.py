"""The fused per-step wrapper entries without a GPU: the inputs of tests/test_gpu_wrap_kernels.py contain every
class of env the rule distinguishes (conditions on the inputs, shown with the torch restatement alone), every refusal of the four entries
(they return before any HIP call), and the four instances of the one kernel template in the built library."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from rodent_amd import hip
from tests import wrap_kernel_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the inputs' classes
@pytest.fixture(scope="module")
def cases():
    return {K: X.inputs(K) for K in X.SLOTS}


def test_the_inputs_hold_every_class_of_env(cases):
    for K, x in cases.items():
        out, plain = X.restate(x, "plain")
        d_env = x["done"] != 0
        over = plain["over"]
        assert (~d_env & ~over).any()                                                    # neither done nor over
        assert (d_env & ~over).any()                                                     # env-done only: truncation 0
        assert (~d_env & over).any() and (d_env & over).any()                            # over alone: truncation 1; both: done 1, truncation 0
        assert out["truncation"][~d_env & over].eq(1).all() and out["truncation"][d_env].eq(0).all() and out["done"][d_env | over].eq(1).all()
        restarted = x["prev_done"] != 0
        assert (restarted & (x["prev_steps"] > 0)).any() and out["steps"][restarted].eq(1).all()      # prev_done: the steps restart
        assert (x["slot_in"] < 0).any() and (x["slot_in"] > K - 1).any()                 # both sides of the slot clamp
        for level, kw in (("restart", {}), ("library", {}), ("library", dict(clip=False, bank_clips=False)), ("sampling", {})):
            _, aux = X.restate(x, level, **kw)
            assert (aux["over_end"] & ~aux["over_len"]).any(), (level, kw)               # over by the clip's end alone
            assert (aux["d"] & (x["slot_in"] < 0)).any() and (x["slot_in"] > K - 1).any()
        assert not X.restate(x, "restart", end_at_clip_end=False)[1]["over_end"].any()
        # the two NaN rows: one env every case ends, one no case ends
        for level in X.LEVELS:
            for ar in (1.0, 2.0):
                d = X.restate(x, level, action_repeat=ar)[1]["d"]
                assert d[X.DONE_ENV] and not d[X.LIVE_ENV]

    x = cases[3]
    out, aux = X.restate(x, "sampling")
    d, slot, cyclic, drawn, nslot = (aux[k] for k in ("d", "slot", "cyclic", "drawn", "nslot"))
    assert (d & (slot == 2) & (X.restate(x, "restart")[1]["nslot"] == 0)).any()          # slot K - 1 wraps to 0
    assert (d & (drawn >= 0) & (drawn != cyclic)).any()                                  # a drawn slot that is not the next one
    q = x["weights"].long()[x["bank_clips"].long()]                                      # [K, N]
    empty = q.sum(0) == 0
    assert empty[list(X.ZERO_BANK_ENVS)].all() and (d & empty).any() and (drawn[empty] == -1).all() and (nslot[empty & d] == cyclic[empty & d]).all()
    mixed = d & (q.min(0).values == 0) & ~empty                                          # a weight-0 entry next to a positive one
    assert mixed.any() and (q[nslot, torch.arange(X.N)][mixed] > 0).all()
    added = out["outcomes"] - x["outcomes"]
    assert (added[:, 1:4].sum(0) > 0).all() and (added[:, 1:4].sum(1) == added[:, 0]).all() and added[:, 4].sum() == X.N
    assert (X.restate(x, "sampling", pose_fail=False)[0]["outcomes"] - x["outcomes"])[:, 1].sum() == 0
    # K = 1: the one entry comes back whatever the slot was
    assert X.restate(cases[1], "sampling")[0]["slot"].eq(0).all()


def test_the_restatement_keeps_nan_payloads(cases):
    x = cases[3]
    out, _ = X.restate(x, "library")
    bits = lambda t: t.contiguous().view(torch.int32)
    assert bits(out["cur"][2])[X.LIVE_ENV, 257] == X.NAN_BITS and bits(out["cur"][1])[X.DONE_ENV, 0] == X.NAN_BITS
    assert not torch.isnan(out["cur"][2][X.DONE_ENV]).any()
    assert X.same_bits(out["cur"][0], out["cur"][0].clone()) and not X.same_bits(out["cur"][0], x["cur"][0])


# ---------------------------------------------------------------------------------------------- refusals
P = 0x1000          # a non-null pointer: every call below is refused before anything is read through it


def _args(level, narr=0, **kw):
    """The argument list of the entry of `level` with every pointer non-null; `kw` replaces arguments by name."""
    names = ["num_envs", "narr", "first", "cur", "widths", "prev_done", "prev_steps", "done", "steps", "truncation", "episode_length", "action_repeat"]
    a = dict(num_envs=4, narr=narr, first=(C.c_void_p * 13)(*[P] * 13), cur=(C.c_void_p * 13)(*[P] * 13), widths=(C.c_int32 * 13)(*[1] * 13),
             prev_done=P, prev_steps=P, done=P, steps=P, truncation=P, episode_length=5.0, action_repeat=1.0)
    i = X.LEVELS.index(level)
    if i >= 1:
        names += ["cur_frame", "bank_frames", "slot_in", "slot_out", "num_slots", "track_len", "end_at_clip_end"]
        a.update(cur_frame=P, bank_frames=P, slot_in=P, slot_out=P, num_slots=2, track_len=10, end_at_clip_end=1)
    if i >= 2:
        names += ["clip", "bank_clips", "clip_lengths"]
        a.update(clip=P, bank_clips=P, clip_lengths=P)
    if i >= 3:
        names += ["num_clips", "pose_fail", "sampling"]
        block = kw.pop("block", hip.RRClipSamplingIO(P, P, P, P, 0))
        a.update(num_clips=3, pose_fail=P, sampling=C.byref(block))
    assert set(kw) <= set(names), kw
    a.update(kw)
    return [a[n] for n in names] + [None]


ENTRY = dict(plain="rr_wrap_episode_autoreset", restart="rr_wrap_clip_restart", library="rr_wrap_clip_library", sampling="rr_wrap_clip_sampling")


def _refused(level, text, **kw):
    lib = hip.lib()
    assert getattr(lib, ENTRY[level])(*_args(level, **kw)) == -1, (level, kw)
    assert lib.rr_last_error().decode() == f"{ENTRY[level]}: {text}", (level, kw, lib.rr_last_error())


@pytest.mark.parametrize("level", X.LEVELS)
def test_common_refusals_of_every_entry(level):
    i = X.LEVELS.index(level)
    required = ["prev_done", "prev_steps", "done", "steps", "truncation"] + (["cur_frame", "bank_frames", "slot_in", "slot_out"] if i >= 1 else [])
    for name in required:
        _refused(level, "bad argument", **{name: None})
    _refused(level, "bad argument", num_envs=0)
    _refused(level, "bad argument", narr=13)
    _refused(level, "bad argument", narr=-1)
    for arr in ("first", "cur"):
        ptrs = (C.c_void_p * 2)(P, None)
        _refused(level, "null array", narr=2, **{arr: ptrs})
    _refused(level, "null array", narr=2, widths=(C.c_int32 * 2)(1, 0))
    if i >= 1:
        _refused(level, "bad argument", track_len=0)
        for k in (0, 65):
            _refused(level, "num_slots must lie in 1 .. 64", num_slots=k)
        _refused(level, "bad argument", num_slots=0, slot_in=None)                       # the order of the checks
        _refused(level, "num_slots must lie in 1 .. 64", num_slots=65, narr=2, first=(C.c_void_p * 2)(P, None))
    if i >= 2:
        _refused(level, "bad argument", clip=None)                                       # bank_clips without clip


def test_refusals_of_the_sampling_entry():
    io = hip.RRClipSamplingIO
    _refused("sampling", "bad argument", sampling=None)
    _refused("sampling", "bad argument", num_clips=0)
    _refused("sampling", "null clip_weights and outcomes", block=io(None, P, P, None, 0))
    _refused("sampling", "clip_weights needs bank_clips, draws_in and draws_out", block=io(P, None, P, P, 0))
    _refused("sampling", "clip_weights needs bank_clips, draws_in and draws_out", block=io(P, P, None, P, 0))
    _refused("sampling", "clip_weights needs bank_clips, draws_in and draws_out", block=io(P, P, P, P, 0), clip=None, bank_clips=None)
    _refused("sampling", "outcomes of several clips need clip", block=io(None, None, None, P, 0), clip=None, bank_clips=None)
    # the order of the checks: num_slots before the block's own, those before the arrays
    _refused("sampling", "num_slots must lie in 1 .. 64", num_slots=0, block=io(None, P, P, None, 0))
    _refused("sampling", "null clip_weights and outcomes", block=io(None, P, P, None, 0), narr=2, first=(C.c_void_p * 2)(P, None))
    _refused("sampling", "null array", narr=2, first=(C.c_void_p * 2)(P, None))


# ---------------------------------------------------------------------------------------------- the built library
# VGPRs of the parent build's kernel of the same level (rr_wrap_kernel, rr_wrap_restart_kernel, rr_wrap_library_kernel,
# rr_wrap_sampling_kernel; their SGPRs were 26 / 36 / 42 / 72): the caps of the four instances
PARENT_VGPR = {0: 8, 1: 8, 2: 8, 3: 8}


def test_four_instances_of_one_template_within_the_parents_registers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    wrap = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_wrap" in k["name"]]
    levels = {}
    for k in wrap:
        m = re.match(r"_Z14rr_wrap_kernelILi(\d)EEv", k["name"])
        assert m, k["name"]                      # an instance of the template: no rr_wrap_restart_kernel / _library_ / _sampling_, no plain function
        print(k["name"], "vgpr", k["vgpr"], "sgpr", k["sgpr"], "scratch", k["scratch"], "lds", k["lds"])
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr_spill"] == 0, k
        levels[int(m.group(1))] = k
    assert len(wrap) == 4 and sorted(levels) == [0, 1, 2, 3]
    for level, k in levels.items():
        assert k["vgpr"] <= PARENT_VGPR[level], (level, k["vgpr"])
