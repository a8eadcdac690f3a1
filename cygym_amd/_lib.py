"""ctypes binding of libcygym_hip.so (the product's only compute path).

There is NO CPU fallback: if the shared library is missing or a call fails, this
module raises.  The CPU oracle under oracle/ is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("CYGYM_SO") or os.path.join(HERE, "libcygym_hip.so")   # CYGYM_SO: A/B a different build

EXPORTS = [
    "cygym_version", "cygym_sizeof", "cygym_last_error", "cygym_create", "cygym_destroy", "cygym_set_config", "cygym_bind", "cygym_derive",
    "cygym_set_snapshot", "cygym_reset", "cygym_randomize", "cygym_step", "cygym_step_range", "cygym_rollout", "cygym_observe",
    "cygym_gen_actions", "cygym_write_actions", "cygym_decode_actions", "cygym_actor_head_decode", "cygym_actor_mlp_decode", "cygym_actor_mlp_decode_tiled", "cygym_mixture_draw", "cygym_coord_ascent_decode", "cygym_coord_ascent_decode_pop", "cygym_dns_decode", "cygym_committee_decode", "cygym_override_decode", "cygym_comm_actor_decode", "cygym_comm_actor_decode_pop", "cygym_comm_gat_decode", "cygym_comm_gat_workspace_bytes", "cygym_hier_decode", "cygym_hier_decode_pop", "cygym_hier_sample_decode", "cygym_hier_loss", "cygym_hier_loss_backward", "cygym_hmarl_decode", "cygym_hmarl_sample_decode", "cygym_hmarl_pack_slots", "cygym_hmarl_decode_pop", "cygym_meta_decode", "cygym_meta_decode_pop", "cygym_meta_select", "cygym_comm_actor_evaluate", "cygym_comm_actor_evaluate_backward", "cygym_comm_gat_evaluate", "cygym_comm_gat_evaluate_backward", "cygym_comm_gat_eval_workspace_bytes", "cygym_critic_tail", "cygym_critic_tail_backward", "cygym_ppo_finish", "cygym_cat_ppo_loss", "cygym_cat_ppo_loss_backward", "cygym_ippo_advantages", "cygym_ippo_ppo_loss", "cygym_ippo_ppo_loss_backward", "cygym_nash_support_enum", "cygym_nash_workspace_bytes", "cygym_step_actor", "cygym_group_actions", "cygym_sample_group_actions", "cygym_fit_forests",
    "cygym_timer_start", "cygym_timer_stop", "cygym_launch_plan",
]


class CygymError(RuntimeError):
    """`code`: the library's return code (include/cygym_abi.h: CYGYM_EINVAL -1, CYGYM_EHIP -2, CYGYM_EUNSUPPORTED -3,
    CYGYM_ENOTBOUND -4), None for errors raised on the Python side."""
    code = None


EINVAL = -1
EUNSUPPORTED = -3


_lib = None


def load():
    """Load the HIP library; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        raise CygymError(
            f"{SO} is missing: build it with `python -m cygym_amd.build` (hipcc --offload-arch=gfx950). "
            "cygym_amd has no CPU fallback.")
    L = C.CDLL(SO)
    H = C.c_void_p
    L.cygym_version.restype = C.c_int
    L.cygym_last_error.restype = C.c_char_p
    L.cygym_last_error.argtypes = [H]
    L.cygym_create.argtypes = [C.POINTER(abi.Topology), C.POINTER(abi.Config), C.c_int32, C.c_int32, C.POINTER(H)]
    L.cygym_destroy.argtypes = [H]
    L.cygym_destroy.restype = None
    L.cygym_set_config.argtypes = [H, C.POINTER(abi.Config)]
    L.cygym_bind.argtypes = [H, C.POINTER(abi.Buffers)]
    L.cygym_set_snapshot.argtypes = [H, C.POINTER(abi.Buffers)]
    L.cygym_derive.argtypes = [H, C.POINTER(abi.Buffers), C.c_void_p]
    L.cygym_reset.argtypes = [H, C.POINTER(abi.Buffers), C.c_void_p, C.c_int32, C.c_void_p]
    L.cygym_randomize.argtypes = [H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.cygym_step.argtypes = [H, C.POINTER(abi.Actions), C.POINTER(abi.Outputs), C.c_void_p]
    L.cygym_step_range.argtypes = [H, C.c_int32, C.c_int32, C.POINTER(abi.Actions), C.POINTER(abi.Outputs), C.c_void_p]
    L.cygym_rollout.argtypes = [H, C.c_int32, C.POINTER(abi.Actions), C.POINTER(abi.Outputs), C.c_void_p]
    L.cygym_observe.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p]
    L.cygym_write_actions.argtypes = [H, C.POINTER(abi.ActionRows), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_decode_actions.argtypes = [H, C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_actor_head_decode.argtypes = [H, C.POINTER(abi.ActorHead), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_actor_mlp_decode.argtypes = [H, C.POINTER(abi.ActorMlp), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_actor_mlp_decode_tiled.argtypes = [H, C.POINTER(abi.ActorMlp), C.POINTER(abi.ActionVectors), C.c_void_p, C.c_int32, C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_mixture_draw.argtypes = [H, C.POINTER(abi.Mixture), C.c_void_p]
    L.cygym_coord_ascent_decode.argtypes = [H, C.POINTER(abi.Critic), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_coord_ascent_decode_pop.argtypes = [H, C.POINTER(abi.Critic), C.POINTER(abi.CriticPop), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_committee_decode.argtypes = [H, C.POINTER(abi.Committee), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_override_decode.argtypes = [H, C.POINTER(abi.ActionVectors), C.c_int32, C.c_void_p, C.c_int32, C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_dns_decode.argtypes = [H, C.POINTER(abi.Critic), C.POINTER(abi.Dns), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_comm_actor_decode.argtypes =[H, C.POINTER(abi.CommActor), C.POINTER(abi.DeviceLogits), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_comm_actor_decode_pop.argtypes = [H, C.POINTER(abi.CommActor), C.POINTER(abi.CommActorPop), C.POINTER(abi.DeviceLogits), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_comm_gat_decode.argtypes = [H, C.POINTER(abi.CommActor), C.POINTER(abi.CommGat), C.POINTER(abi.DeviceLogits), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_comm_gat_workspace_bytes.argtypes = [H, C.c_int32]
    L.cygym_comm_gat_workspace_bytes.restype = C.c_uint64
    L.cygym_hier_decode.argtypes = [H, C.POINTER(abi.HierNet), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_hier_decode_pop.argtypes = [H, C.POINTER(abi.HierNet), C.POINTER(abi.HierPop), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_hier_sample_decode.argtypes = [H, C.POINTER(abi.HierNet), C.POINTER(abi.HierSample), C.POINTER(abi.ActionVectors), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_hier_loss.argtypes = [H, C.POINTER(abi.HierLoss), C.c_void_p]
    L.cygym_hier_loss_backward.argtypes = [H, C.POINTER(abi.HierLoss), C.c_void_p]
    L.cygym_hmarl_decode.argtypes = [H, C.POINTER(abi.Hmarl), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_hmarl_sample_decode.argtypes = [H, C.POINTER(abi.Hmarl), C.POINTER(abi.HmarlTrain), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_hmarl_pack_slots.argtypes = [H, C.POINTER(abi.Hmarl), C.c_int32, C.POINTER(abi.HmarlSlot)]
    L.cygym_hmarl_decode_pop.argtypes = [H, C.POINTER(abi.Hmarl), C.POINTER(abi.HmarlPop), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_meta_decode.argtypes = [H, C.POINTER(abi.Meta), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_meta_decode_pop.argtypes = [H, C.POINTER(abi.Meta), C.POINTER(abi.MetaPop), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_meta_select.argtypes =[H, C.POINTER(abi.MetaSelect), C.c_void_p]
    L.cygym_comm_actor_evaluate.argtypes = [H, C.POINTER(abi.CommEval), C.c_void_p]
    L.cygym_comm_actor_evaluate_backward.argtypes = [H, C.POINTER(abi.CommEval), C.c_void_p]
    L.cygym_comm_gat_evaluate.argtypes = [H, C.POINTER(abi.CommGatEval), C.c_void_p]
    L.cygym_comm_gat_evaluate_backward.argtypes = [H, C.POINTER(abi.CommGatEval), C.c_void_p]
    L.cygym_comm_gat_eval_workspace_bytes.argtypes = [H, C.c_int32, C.c_int32, C.c_int32]
    L.cygym_comm_gat_eval_workspace_bytes.restype = C.c_uint64
    L.cygym_critic_tail.argtypes = [H, C.POINTER(abi.CriticTail), C.c_void_p]
    L.cygym_critic_tail_backward.argtypes = [H, C.POINTER(abi.CriticTail), C.c_void_p]
    L.cygym_ppo_finish.argtypes = [H, C.POINTER(abi.PpoFinish), C.c_void_p]
    L.cygym_cat_ppo_loss.argtypes = [H, C.POINTER(abi.CatPpo), C.c_void_p]
    L.cygym_cat_ppo_loss_backward.argtypes = [H, C.POINTER(abi.CatPpo), C.c_void_p]
    L.cygym_ippo_advantages.argtypes = [H, C.POINTER(abi.IppoAdv), C.c_void_p]
    L.cygym_ippo_ppo_loss.argtypes = [H, C.POINTER(abi.IppoHead), C.c_void_p]
    L.cygym_ippo_ppo_loss_backward.argtypes = [H, C.POINTER(abi.IppoHead), C.c_void_p]
    L.cygym_nash_support_enum.argtypes = [H, C.POINTER(abi.NashDesc), C.c_void_p]
    L.cygym_nash_workspace_bytes.argtypes = [C.POINTER(abi.NashDesc)]
    L.cygym_nash_workspace_bytes.restype = C.c_uint64
    L.cygym_step_actor.argtypes = [H, C.POINTER(abi.Actions), C.POINTER(abi.Outputs), C.POINTER(abi.ActorMlp), C.POINTER(abi.ActionVectors),
                                   C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_group_actions.argtypes = [H, C.POINTER(abi.DeviceTypes), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_sample_group_actions.argtypes = [H, C.POINTER(abi.DeviceLogits), C.POINTER(abi.Actions), C.c_void_p]
    L.cygym_fit_forests.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.cygym_gen_actions.argtypes = [H, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_void_p]
    L.cygym_timer_start.argtypes = [H, C.c_void_p]
    L.cygym_timer_stop.argtypes = [H, C.c_void_p, C.POINTER(C.c_float)]
    L.cygym_launch_plan.argtypes = [H, C.POINTER(C.c_int32)]
    if L.cygym_version() != abi.ABI_VERSION:
        raise CygymError(f"ABI mismatch: library {L.cygym_version()} vs python {abi.ABI_VERSION}")
    L.cygym_sizeof.argtypes = [C.c_int32]
    for which, st in enumerate((abi.Topology, abi.Config, abi.Buffers, abi.Actions, abi.Outputs, abi.ActionRows, abi.ActionVectors, abi.ActorHead, abi.ActorMlp, abi.DeviceTypes, abi.DeviceLogits, abi.Critic, abi.CommActor)):
        if L.cygym_sizeof(which) != C.sizeof(st):
            raise CygymError(f"ABI struct {st.__name__}: library {L.cygym_sizeof(which)} bytes vs python {C.sizeof(st)}")
    if L.cygym_sizeof(14) != C.sizeof(abi.CommEval):   # (index 13 is unassigned)
        raise CygymError(f"ABI struct CommEval: library {L.cygym_sizeof(14)} bytes vs python {C.sizeof(abi.CommEval)}")
    if L.cygym_sizeof(16) != C.sizeof(abi.CriticTail):   # (index 15 is unassigned)
        raise CygymError(f"ABI struct CriticTail: library {L.cygym_sizeof(16)} bytes vs python {C.sizeof(abi.CriticTail)}")
    if L.cygym_sizeof(17) != C.sizeof(abi.HierNet):
        raise CygymError(f"ABI struct HierNet: library {L.cygym_sizeof(17)} bytes vs python {C.sizeof(abi.HierNet)}")
    for which, st in ((19, abi.HierSample), (20, abi.HierLoss), (21, abi.Hmarl), (23, abi.Meta), (25, abi.MetaSelect), (27, abi.PpoFinish), (28, abi.CatPpo), (29, abi.HmarlTrain),
                      (31, abi.Dns), (33, abi.Mixture), (35, abi.CommGat), (37, abi.CommGatEval),
                      (39, abi.IppoAdv), (40, abi.IppoHead), (42, abi.Committee), (44, abi.CriticPop), (46, abi.CommActorPop), (48, abi.HierPop), (50, abi.MetaPop), (52, abi.NashDesc),
                      (54, abi.HmarlPop), (55, abi.HmarlSlot)):   # (indices 18, 22, 24, 26, 30, 32, 34, 36, 38, 41, 43, 45, 47, 49, 51 and 53 are unassigned)
        if L.cygym_sizeof(which) != C.sizeof(st):
            raise CygymError(f"ABI struct {st.__name__}: library {L.cygym_sizeof(which)} bytes vs python {C.sizeof(st)}")
    _lib = L
    return L


def check(rc: int, handle=None, what: str = ""):
    if rc != 0:
        msg = load().cygym_last_error(handle)
        err = CygymError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        err.code = int(rc)
        raise err
