"""Path-EIG evaluator: the planner's scoring of candidate action sequences
(tester_gaussians_navigation.py:1664-1727) on top of the batched Fisher scorer.

Reference loop, per path: roll the camera forward one action at a time (`compute_next_campos`,
models/SLAM/utils/slam_external.py:44-65), call `compute_Hessian` at EVERY step, and on every
`acc_H_train_every`-th step add `log sum(cur_H / (H_path + lambda))` to the path value and fold `cur_H` into `H_path`.
Only the accumulation steps influence the point term, and step m of a path needs the cur_H of its steps < m, so the batched
form runs in rounds: round m scores the m-th accumulation step of ALL paths in one `fr_fisher_views` call with per-view
weights (`H_inv_view_stride`) and per-view `out_H` blocks, then updates every path's `H_path`.
Every step also adds `path_pose_weight * log(det(pose_H))`.  The reference's pose_H is eye(6), a placeholder, so that term is
zero; `evaluate_paths(..., pose_fisher=True)` puts the camera-pose Fisher information there (`FisherScorer.pose_fisher`, all
steps of all paths in one batched call).
"""
import numpy as np
import torch


def compute_next_campos(cam_H, action_id, forward_step_size=0.065, turn_angle=10.):
    """One agent action applied to a camera-to-world matrix (float64, like the reference).
    1: forward along +z of the camera; 2 / 3: yaw by -/+ turn_angle degrees about the camera's y axis; else no-op."""
    next_H = np.array(cam_H, dtype=np.float64, copy=True)
    if action_id == 1:
        next_H[:3, 3] = cam_H[:3, 3] + cam_H[:3, :3] @ np.array([0.0, 0.0, forward_step_size])
    elif action_id in (2, 3):
        a = np.deg2rad(turn_angle)
        s = -np.sin(a) if action_id == 2 else np.sin(a)
        R = np.array([[np.cos(a), 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, np.cos(a)]])
        next_H[:3, :3] = cam_H[:3, :3] @ R
    return next_H


def rollout(start_c2w, actions, forward_step_size=0.065, turn_angle=10.):
    H = np.array(start_c2w, dtype=np.float64)
    out = np.zeros((len(actions), 4, 4))
    for t, a in enumerate(actions):
        H = compute_next_campos(H, int(a), forward_step_size, turn_angle)
        out[t] = H
    return out


def pose_log_det(pose_H, pose_reg=0.0):
    """log det(pose_H + pose_reg I) of a [..., 6, 6] batch, in float64 (as NumPy).  A determinant <= 0 gives -inf: the
    reference's torch.log(torch.linalg.det(pose_H)) of a singular matrix."""
    M = torch.as_tensor(pose_H).detach().to("cpu", torch.float64).numpy()
    M = M + float(pose_reg) * np.eye(6)
    sign, logabs = np.linalg.slogdet(M)
    return np.where(sign > 0, logabs, -np.inf)


def evaluate_paths(scorer, start_c2w, path_actions, final_EIGs, H_train, *, forward_step_size=0.065, turn_angle=10.,
                   H_reg_lambda=0.1, acc_H_train_every=5, path_point_weight=1.0, path_pose_weight=0.0,
                   path_end_weight=0.0, vol_weighted_H=False, gs_pts_cnt=1.0, cam_height=None, pose_fisher=False, pose_reg=0.0):
    """Returns the list of total_path_EIG values (tester 1713-1718).  `scorer` is a FisherScorer of the current map,
    `H_train` the [P,C] keyframe accumulator.
    The reference adds `path_pose_weight * log(det(pose_H))` at EVERY step of a path (tester 1697-1701), with the identity
    placeholder as pose_H: a zero term.  pose_fisher=False keeps that (the term is left out; the result is what it always was).
    pose_fisher=True takes pose_H from `scorer.pose_fisher` -- the camera-pose Fisher information of the step's view, every step of
    every path in one batched call -- and adds `path_pose_weight * log det(pose_H + pose_reg I)` (float64) per step, in the
    reference's order of the terms; a determinant <= 0 adds -inf, as the reference's log(det) of a singular matrix would."""
    dev = scorer.dev
    P, C = scorer.P, scorer.columns
    start = np.array(start_c2w, dtype=np.float64, copy=True)
    if cam_height is not None:
        start[1, 3] = cam_height
    n_paths = len(path_actions)
    # accumulation steps: 1-based step s with (s + 1) % acc == 0
    acc_steps = [[s for s in range(1, len(a) + 1) if (s + 1) % acc_H_train_every == 0] for a in path_actions]
    poses = [rollout(start, a, forward_step_size, turn_angle) for a in path_actions]
    totals = [0.0] * n_paths
    point_terms = [[] for _ in range(n_paths)]
    H_path = {i: H_train.clone() for i in range(n_paths) if acc_steps[i]}
    rounds = max((len(s) for s in acc_steps), default=0)
    for m in range(rounds):
        active = [i for i in range(n_paths) if len(acc_steps[i]) > m]
        c2w = np.stack([poses[i][acc_steps[i][m] - 1] for i in active])
        w2c = torch.from_numpy(np.linalg.inv(c2w)).float().to(dev)
        H_inv = torch.stack([torch.reciprocal(H_path[i] + H_reg_lambda) for i in active])
        if vol_weighted_H:
            H_inv = H_inv / gs_pts_cnt
        last_round = {i: len(acc_steps[i]) == m + 1 for i in active}
        cur = torch.zeros((len(active), P, C), dtype=torch.float32, device=dev)
        res = scorer.run(w2c, H_inv=H_inv, H_inv_per_view=True, out_H=cur, out_H_per_view=True)
        point_EIG = torch.log(res["scores"]).cpu().numpy()
        for k, i in enumerate(active):
            totals[i] += path_point_weight * float(point_EIG[k])
            point_terms[i].append(path_point_weight * float(point_EIG[k]))
            if not last_round[i]:
                H_path[i] = H_path[i] + cur[k]
    if pose_fisher:
        # every step of every path in one call (the scorer splits it by its launch limit); the terms summed in the reference's order:
        # per step the pose term, then the point term where the step is an accumulation step
        all_c2w = np.concatenate([poses[i] for i in range(n_paths)]) if n_paths else np.zeros((0, 4, 4))
        pose_terms = np.zeros(0)
        if len(all_c2w):
            w2c_all = torch.from_numpy(np.linalg.inv(all_c2w)).float().to(dev)
            pose_terms = path_pose_weight * pose_log_det(scorer.pose_fisher(w2c_all), pose_reg)
        k0 = 0
        for i in range(n_paths):
            total = 0.0
            acc = set(acc_steps[i])
            pts = iter(point_terms[i])
            for s in range(1, len(path_actions[i]) + 1):
                total += float(pose_terms[k0 + s - 1])
                if s in acc:
                    total += next(pts)
            totals[i] = total
            k0 += len(path_actions[i])
    out = []
    for i in range(n_paths):
        n = max(len(path_actions[i]), 1)
        if path_end_weight > 0:
            out.append(totals[i] / n + path_end_weight * float(final_EIGs[i]))
        else:
            out.append((totals[i] + float(final_EIGs[i])) / n)
    return out
