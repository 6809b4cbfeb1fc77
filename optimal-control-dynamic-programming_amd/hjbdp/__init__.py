"""hjbdp - host side of libhjbdp, the MI355X-native Bellman-backup path of
abdolrezat/Optimal-Control-Dynamic-Programming.

The classes keep the reference's names and methods so its scripts read the same:

    from hjbdp import Dynamic_Solver
    objA = Dynamic_Solver(); objA.run(); objA.get_optimal_path()

All sweeps run in the HIP library (hjbdp/libhjbdp.so, C ABI in include/hjbdp.h);
there is no CPU fallback.
"""
from . import _abi
from .core import ActuatorRollout, Backup, ControlLookaheadRollout, DeviceBuffer, HjbError, MultiBackup, RankSlab, Rollout, attitude_linear_response, campaign_hist_reduce, campaign_pair_reduce, campaign_quantiles, campaign_reduce, campaign_tail_mean, control_lookahead_host, device_count, device_mem_info, greedy_host, load_library, lookahead_campaign_host, lookahead_host, noise_draw, noise_thresholds, policy_lookup, solve_batch, solve_many, suggest_axis_order
from .problem import ProblemSpec, Term, permute_state_axes
from .disturbance import actuator_nodes, box_nodes, gaussian_nodes
from .dynamic_solver import Dynamic_Solver
from .solver_position import Solver_position
from .solver_attitude import Solver_attitude
from .solver_pos_att import Solver_pos_att

__all__ = ["ActuatorRollout", "Backup", "ControlLookaheadRollout", "DeviceBuffer", "device_mem_info", "MultiBackup", "RankSlab", "Rollout", "HjbError", "ProblemSpec", "Term", "permute_state_axes", "Dynamic_Solver", "Solver_position", "Solver_attitude", "Solver_pos_att", "attitude_linear_response", "campaign_reduce", "campaign_hist_reduce", "campaign_pair_reduce", "campaign_quantiles", "campaign_tail_mean", "device_count", "load_library", "greedy_host", "lookahead_host", "lookahead_campaign_host", "control_lookahead_host", "noise_draw", "noise_thresholds", "policy_lookup", "solve_batch", "solve_many", "suggest_axis_order", "gaussian_nodes", "box_nodes", "_abi"]
