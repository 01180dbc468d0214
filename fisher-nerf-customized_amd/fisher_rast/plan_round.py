"""The planning round after `global_planning`: goals -> paths -> action lists -> path values -> the best path
(tester_gaussians_navigation.py: action_planning 2207-2332, plan_best_path 1628-1736 without global_planning and compute_H_train).

`action_planning` is `setup_start` + `PathPlanOps.plan_actions`: one cost field, every goal's path and action list on the device, one
host read.  `plan_best_path` sorts the goals by EIG, plans, and scores at most 21 paths with `evaluate_paths`, fed by the poses
`plan_actions` left on the device -- nothing is rolled out or inverted on the host.

What differs from the reference: a kept path with no action makes the reference divide by zero; here it is
left out of the scoring and listed in the result.  The reference pairs the i-th KEPT path with EIGs[i] -- it zips the filtered lists
against the unfiltered EIGs -- which is kept; `align_EIGs=True` pairs a path with its own goal's EIG instead.

The object round (tester 1738-1818): `action_planning_object_adv` is `setup_start` + `PathPlanOps.plan_actions_object`, and
`plan_best_object_path` chains `GoalSelectOps.global_object_planning`, the object map's H_train, the adv follower and the scoring of at
most 21 paths.  What differs there is said in INTEGRATION.md section 4b.3; in short: for criteria "fisher" the reference's
path_evaluation overwrites every point_EIG with 0 and takes log det of a placeholder eye(6), so a path's value is
object_path_end_weight * final_EIG (final_EIG / len when that weight is 0) -- computed here on the host, with no Hessian launched.
Not rebuilt: action_planning_object (superseded by _adv in the reference), path_object_evaluation (its call is commented out there),
num_uniform_H_train, draw_final_map, the PNG and pickle outputs.
"""
import numpy as np
import torch

from . import path_eval

MAX_SCORED_PATHS = 21               # tester 1669-1672: `valid_path > 20` breaks after 21 paths

_STEP_KEYS = ("forward_step_size", "turn_angle", "queue_size")


def _step_cfg(cfg):
    """forward_step_size, turn_angle, queue_size from keyword arguments or a slam_config-shaped mapping
    (slam_config["forward_step_size"], ["turn_angle"], ["policy"]["planning_queue_size"])"""
    cfg = dict(cfg)
    if "queue_size" not in cfg:
        if "planning_queue_size" in cfg:
            cfg["queue_size"] = cfg["planning_queue_size"]
        elif "policy" in cfg and "planning_queue_size" in cfg["policy"]:
            cfg["queue_size"] = cfg["policy"]["planning_queue_size"]
    missing = [k for k in _STEP_KEYS if k not in cfg]
    if missing:
        raise ValueError(f"the step configuration lacks {missing}")
    return {k: cfg[k] for k in _STEP_KEYS}


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def action_planning(planner, global_points, current_agent_pose, gaussian_points, t, return_plan=False, **step_cfg):
    """NavTester.action_planning on a planner with PathPlanOps: (valid_global_points, path_actions, paths_arr), or the ActionPlan
    that holds them with return_plan=True.  step_cfg: forward_step_size, turn_angle, queue_size (or a slam_config's keys)."""
    step = _step_cfg(step_cfg)
    current_agent_pose = _np(current_agent_pose)
    current_agent_pos = current_agent_pose[:3, 3]
    start = planner._plan_to_map(current_agent_pos[[0, 2]])[[1, 0]]              # convert_to_map on the held map centre; from x-z to z-x
    planner.setup_start(start, gaussian_points, t)
    plan = planner.plan_actions(_np(global_points), current_agent_pose, **step)
    return plan if return_plan else plan.triple()


class BestPath(tuple):
    """plan_best_path's result: the reference's (best_path, best_map_path, best_goal, best_world_path, best_global_path) and, sixth,
    the list of totals; as attributes also `plan` (the ActionPlan), `scored` (positions in the kept lists that were scored, in order),
    `skipped_empty` (kept paths without an action, which the reference cannot score), `best_index` (position in the kept lists or
    None), `global_points` and `EIGs` as sorted."""


def plan_best_path(scorer_or_slam, planner, global_points, EIGs, H_train, current_agent_pose, gaussian_points, t, cfg, align_EIGs=False):
    """The part of NavTester.plan_best_path after global_planning and compute_H_train.  scorer_or_slam: a FisherScorer of the map, or a
    SLAM object with FisherOps installed.  cfg: a mapping with forward_step_size, turn_angle, queue_size (or planning_queue_size) and,
    optionally, evaluate_paths' H_reg_lambda, acc_H_train_every, path_point_weight, path_pose_weight, path_end_weight, vol_weighted_H,
    gs_pts_cnt, pose_fisher, pose_reg."""
    scorer = scorer_or_slam._scorer() if hasattr(scorer_or_slam, "_scorer") else scorer_or_slam
    if not (hasattr(scorer, "run") and hasattr(scorer, "dev")):
        raise ValueError("plan_best_path: needs a FisherScorer or a SLAM object with FisherOps installed")
    EIGs = _np(EIGs).reshape(-1)
    global_points = _np(global_points).reshape(-1, 4, 4)
    if len(EIGs) != len(global_points):
        raise ValueError(f"{len(global_points)} goals, {len(EIGs)} EIGs")
    sort_index = np.argsort(EIGs)[::-1]
    global_points = global_points[sort_index]
    EIGs = EIGs[sort_index]
    plan = action_planning(planner, global_points, current_agent_pose, gaussian_points, t, return_plan=True, **_step_cfg(cfg))
    kept = list(range(len(plan.kept_index)))[:MAX_SCORED_PATHS]
    skipped = [i for i in kept if len(plan.path_actions[i]) == 0]
    scored = [i for i in kept if len(plan.path_actions[i]) > 0]
    finals = [float(EIGs[plan.kept_index[i]] if align_EIGs else EIGs[i]) for i in scored]
    kw = {k: cfg[k] for k in ("H_reg_lambda", "acc_H_train_every", "path_point_weight", "path_pose_weight", "path_end_weight", "vol_weighted_H",
                              "gs_pts_cnt", "pose_fisher", "pose_reg") if k in cfg}
    totals = []
    if scored:
        totals = path_eval.evaluate_paths(scorer, _np(current_agent_pose), [plan.path_actions[i] for i in scored], finals, H_train,
                                          poses_w2c=plan.kept_w2c(scored), **kw)
    best, best_EIG = None, -1.
    for i, total in zip(scored, totals):                        # the first maximum above -1 (tester 1721)
        if total > best_EIG:
            best, best_EIG = i, total
    if best is None:
        five = (None, None, None, None, None)
    else:
        five = (plan.path_actions[best], plan.map_path[best], plan.valid_global_points[best], plan.world_path[best], plan.paths_arr[best])
    out = BestPath(five + (list(totals),))
    out.plan, out.scored, out.skipped_empty, out.best_index, out.global_points, out.EIGs = plan, scored, skipped, best, global_points, EIGs
    return out


# ---- the object round ------------------------------------------------------------------------------------------------------------------

def _object_step_cfg(cfg):
    """forward_step_size and turn_angle from keyword arguments or a slam_config-shaped mapping (the adv follower has no queue size)"""
    missing = [k for k in _STEP_KEYS[:2] if k not in cfg]
    if missing:
        raise ValueError(f"the step configuration lacks {missing}")
    return {k: cfg[k] for k in _STEP_KEYS[:2]}


def action_planning_object_adv(planner, global_points, current_agent_pose, gaussian_points, t, return_plan=False, **step_cfg):
    """NavTester.action_planning_object_adv on a planner with PathPlanOps: (valid_global_points, path_actions, paths_arr) -- the
    pruned paths -- or the ObjectActionPlan that holds them with return_plan=True.  step_cfg: forward_step_size, turn_angle."""
    step = _object_step_cfg(step_cfg)
    current_agent_pose = _np(current_agent_pose)
    start = planner._plan_to_map(current_agent_pose[[0, 2], 3])[[1, 0]]
    planner.setup_start(start, gaussian_points, t)
    plan = planner.plan_actions_object(_np(global_points), current_agent_pose, **step)
    return plan if return_plan else plan.triple()


def fisher_object_path_value(final_EIG, n_actions, object_path_end_weight=0.0):
    """total_path_EIG of path_evaluation (tester 1900-1964) as the reference computes it today: point_EIG is overwritten with 0
    (1933, 1940) and pose_EIG is log det of the object map's placeholder eye(6), 0 -- what is left is the end term"""
    final = float(final_EIG.item() if hasattr(final_EIG, "item") else final_EIG)
    if object_path_end_weight > 0:
        return float(object_path_end_weight) * final
    return final / int(n_actions)


class BestObjectPath(tuple):
    """plan_best_object_path's result: the reference's (best_path, best_map_path, best_goal, best_world_path, best_global_path,
    global_points, EIGs); as attributes also `plan` (the ObjectActionPlan), `totals`, `scored` (positions in the kept lists, in
    order), `best_index` (position in the kept lists or None), `candidate_object_pose`."""


def plan_best_object_path(obj_slam, slam, planner, current_agent_pose, expansion, t, cfg, criteria, H_train=None):
    """NavTester.plan_best_object_path (tester 1738-1818) on a planner with GoalSelectOps and PathPlanOps.  obj_slam / slam: the object
    and the scene SLAM objects (`gaussian_points`; obj_slam's pose_eval / pose_eval_popgs, compute_H_train_popgs and, optionally,
    pose_proposal).  cfg: a mapping with forward_step_size, turn_angle and, optionally, object_path_end_weight, path_end_weight,
    path_point_weight, acc_H_train_every, lam, K.  criteria: "fisher", or "topt" / "dopt".  H_train: the POp-GS prior when the
    caller already holds it (not read for "fisher")."""
    crit = str(criteria).lower()
    current_agent_pose = _np(current_agent_pose)
    current_agent_pos = current_agent_pose[:3, 3]
    pose_proposal_fn = getattr(obj_slam, "pose_proposal", None)
    if crit == "fisher":
        res = planner.global_object_planning(obj_slam.pose_eval, obj_slam.gaussian_points, slam.gaussian_points, pose_proposal_fn, expansion=expansion,
                                             visualize=False, agent_pose=current_agent_pos)
    else:
        res = planner.global_object_planning(obj_slam.pose_eval_popgs, obj_slam.gaussian_points, slam.gaussian_points, pose_proposal_fn,
                                             expansion=expansion, visualize=False, agent_pose=current_agent_pos, criterion=criteria)
    global_points, EIGs, _, candidate_object_pose = res
    EIGs = _np(EIGs).reshape(-1)
    global_points = _np(global_points).reshape(-1, 4, 4)
    sort_index = np.argsort(EIGs)[::-1]
    global_points = global_points[sort_index]
    EIGs = EIGs[sort_index]
    plan = action_planning_object_adv(planner, global_points, current_agent_pose, slam.gaussian_points, t, return_plan=True, **_object_step_cfg(cfg))
    scored = list(range(len(plan.kept_index)))[:MAX_SCORED_PATHS]
    finals = [float(EIGs[i]) for i in scored]                    # the i-th KEPT path with EIGs[i], as the reference zips them
    w_end = float(cfg.get("object_path_end_weight", 0.0))
    if crit == "fisher":
        totals = [fisher_object_path_value(f, len(plan.path_actions[i]), w_end) for i, f in zip(scored, finals)]
        floor = -1.                                              # tester 1891
    else:
        if H_train is None and scored:
            H_train = obj_slam.compute_H_train_popgs()
        kw = {k: cfg[k] for k in ("lam", "K", "acc_H_train_every", "path_point_weight", "path_end_weight") if k in cfg}
        totals = []
        if scored:
            totals = path_eval.evaluate_paths_popgs(obj_slam, current_agent_pose, [plan.path_actions[i] for i in scored], finals, H_train,
                                                    criterion=crit, object_path_end_weight=w_end, poses_w2c=plan.kept_w2c(scored), **kw)
        floor = -float("inf")                                    # tester 2114
    best, best_EIG = None, floor
    for i, total in zip(scored, totals):                         # the first maximum above the floor
        if total > best_EIG:
            best, best_EIG = i, total
    if best is None:
        five = (None, None, None, None, None)
    else:
        five = (plan.path_actions[best], plan.map_path[best], plan.valid_global_points[best], plan.world_path[best], plan.paths_arr[best])
    out = BestObjectPath(five + (global_points, EIGs))
    out.plan, out.totals, out.scored, out.best_index, out.candidate_object_pose = plan, list(totals), scored, best, candidate_object_pose
    return out
