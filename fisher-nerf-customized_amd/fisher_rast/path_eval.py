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
`evaluate_paths_popgs` (below) is the same round structure for the POp-GS variant of the loop (tester 2109-2204).
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


def rollout_device(start_c2w, path_actions, forward_step_size=0.065, turn_angle=10., *, cam_height=None, queue_size=None, device=None,
                   return_c2w=False):
    """The roll-out and the inversion of every pose on the device (fisher_occ.h: fr_rollout_actions, binary64, each inverse rounded once
    to binary32): action lists -> (w2c float32 [n_paths, Q, 4, 4] on the device, zeros behind a list; the lists' lengths).
    Q = queue_size or the longest list; with return_c2w also the poses, float64 [n_paths, Q, 4, 4].  What `poses_w2c=` of
    evaluate_paths / evaluate_paths_popgs takes for action lists that do not come from `plan_actions`."""
    import ctypes
    from . import _lib
    lengths = [len(a) for a in path_actions]
    Q = int(queue_size) if queue_size is not None else max(lengths + [1])
    if not 1 <= Q <= _lib.FR_ACTION_MAX_QUEUE:
        raise ValueError(f"the longest action list may have 1 .. {_lib.FR_ACTION_MAX_QUEUE} actions, got {Q}")
    if max(lengths + [0]) > Q:
        raise ValueError(f"an action list has {max(lengths)} actions, queue_size is {Q}")
    start = np.array(start_c2w.detach().cpu().numpy() if isinstance(start_c2w, torch.Tensor) else start_c2w, dtype=np.float64)
    if start.shape != (4, 4):
        raise ValueError(f"start_c2w must be 4 x 4, got {start.shape}")
    if cam_height is not None:
        start[1, 3] = cam_height
    n = len(path_actions)
    acts = np.zeros((n, Q), np.uint8)
    for i, a in enumerate(path_actions):
        a = np.asarray(a, dtype=np.int64).reshape(-1)
        if len(a) and (a.min() < 0 or a.max() > 255):
            raise ValueError("actions must fit a byte")
        acts[i, :len(a)] = a
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    w2c = torch.empty((n, Q, 4, 4), dtype=torch.float32, device=dev)
    c2w = torch.empty((n, Q, 4, 4), dtype=torch.float64, device=dev) if return_c2w else None
    if n:
        lib = _lib.load()
        acts_d = torch.from_numpy(acts).to(dev)
        lens_d = torch.tensor(lengths, dtype=torch.int32).to(dev)
        start_a = (ctypes.c_double * 16)(*[float(v) for v in start.reshape(-1)])
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.fr_rollout_actions(start_a, acts_d.data_ptr(), lens_d.data_ptr(), n, Q, float(forward_step_size), float(turn_angle),
                                              w2c.data_ptr(), None if c2w is None else c2w.data_ptr(), stream), "fr_rollout_actions")
    return (w2c, lengths, c2w) if return_c2w else (w2c, lengths)


def _check_poses_w2c(poses_w2c, path_actions, dev):
    """the device poses of `poses_w2c=`: [n_paths, Q, 4, 4] float32 on the scorer's device, Q at least the longest list"""
    if not isinstance(poses_w2c, torch.Tensor):
        raise ValueError("poses_w2c must be a torch tensor [n_paths, Q, 4, 4] on the device")
    n, longest = len(path_actions), max([len(a) for a in path_actions] + [0])
    if poses_w2c.dim() != 4 or tuple(poses_w2c.shape[2:]) != (4, 4) or poses_w2c.shape[0] != n or poses_w2c.shape[1] < longest:
        raise ValueError(f"poses_w2c has shape {tuple(poses_w2c.shape)}, expected [{n}, Q >= {longest}, 4, 4]")
    if poses_w2c.dtype != torch.float32:
        raise ValueError(f"poses_w2c must be float32, got {poses_w2c.dtype}")
    if poses_w2c.device != torch.device(dev):
        raise ValueError(f"poses_w2c lives on {poses_w2c.device}, the map on {dev}")
    return poses_w2c


def _gather_w2c(poses_w2c, pairs):
    """poses_w2c[path, step - 1] for (path, step) pairs, gathered on the device"""
    idx = torch.tensor([[i, s - 1] for i, s in pairs], dtype=torch.long).to(poses_w2c.device)
    return poses_w2c[idx[:, 0], idx[:, 1]].contiguous()


def pose_log_det(pose_H, pose_reg=0.0):
    """log det(pose_H + pose_reg I) of a [..., 6, 6] batch, in float64 (as NumPy).  A determinant <= 0 gives -inf: the
    reference's torch.log(torch.linalg.det(pose_H)) of a singular matrix."""
    M = torch.as_tensor(pose_H).detach().to("cpu", torch.float64).numpy()
    M = M + float(pose_reg) * np.eye(6)
    sign, logabs = np.linalg.slogdet(M)
    return np.where(sign > 0, logabs, -np.inf)


def evaluate_paths(scorer, start_c2w, path_actions, final_EIGs, H_train, *, forward_step_size=0.065, turn_angle=10.,
                   H_reg_lambda=0.1, acc_H_train_every=5, path_point_weight=1.0, path_pose_weight=0.0,
                   path_end_weight=0.0, vol_weighted_H=False, gs_pts_cnt=1.0, cam_height=None, pose_fisher=False, pose_reg=0.0,
                   poses_w2c=None):
    """Returns the list of total_path_EIG values (tester 1713-1718).  `scorer` is a FisherScorer of the current map,
    `H_train` the [P,C] keyframe accumulator.
    The reference adds `path_pose_weight * log(det(pose_H))` at EVERY step of a path (tester 1697-1701), with the identity
    placeholder as pose_H: a zero term.  pose_fisher=False keeps that (the term is left out; the result is what it always was).
    pose_fisher=True takes pose_H from `scorer.pose_fisher` -- the camera-pose Fisher information of the step's view, every step of
    every path in one batched call -- and adds `path_pose_weight * log det(pose_H + pose_reg I)` (float64) per step, in the
    reference's order of the terms; a determinant <= 0 adds -inf, as the reference's log(det) of a singular matrix would.
    poses_w2c: a device tensor float32 [n_paths, Q, 4, 4] holding the inverse of the pose after every action of every path
    (`PathPlanOps.plan_actions`' w2c, or `rollout_device`); with it nothing is rolled out or inverted on the host, and `start_c2w`,
    the step sizes and `cam_height` are not read."""
    dev = scorer.dev
    P, C = scorer.P, scorer.columns
    start = np.array(start_c2w, dtype=np.float64, copy=True)
    if cam_height is not None:
        start[1, 3] = cam_height
    n_paths = len(path_actions)
    # accumulation steps: 1-based step s with (s + 1) % acc == 0
    acc_steps = [[s for s in range(1, len(a) + 1) if (s + 1) % acc_H_train_every == 0] for a in path_actions]
    if poses_w2c is not None:
        poses_w2c = _check_poses_w2c(poses_w2c, path_actions, dev)
    else:
        poses = [rollout(start, a, forward_step_size, turn_angle) for a in path_actions]
    totals = [0.0] * n_paths
    point_terms = [[] for _ in range(n_paths)]
    H_path = {i: H_train.clone() for i in range(n_paths) if acc_steps[i]}
    rounds = max((len(s) for s in acc_steps), default=0)
    for m in range(rounds):
        active = [i for i in range(n_paths) if len(acc_steps[i]) > m]
        if poses_w2c is not None:
            w2c = _gather_w2c(poses_w2c, [(i, acc_steps[i][m]) for i in active])
        else:
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
        pose_terms = np.zeros(0)
        if poses_w2c is not None:
            steps = [(i, s) for i in range(n_paths) for s in range(1, len(path_actions[i]) + 1)]
            w2c_all = _gather_w2c(poses_w2c, steps) if steps else None
        else:
            all_c2w = np.concatenate([poses[i] for i in range(n_paths)]) if n_paths else np.zeros((0, 4, 4))
            w2c_all = torch.from_numpy(np.linalg.inv(all_c2w)).float().to(dev) if len(all_c2w) else None
        if w2c_all is not None:
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


# ---- POp-GS path evaluation (tester_gaussians_navigation.py:2109-2204) ------------------------------------------------------
# The reference calls `estimate_diag_JtJ_simple` at EVERY step of every path -- K probes through autograd each -- scores the step
# with T-opt or D-opt against the path's prior, and uses the result only on every `acc_H_train_every`-th step, where it also
# folds the estimate into the prior.  Here only the accumulation steps are computed, in rounds as `evaluate_paths` runs them:
# round m = ONE probe launch for the m-th accumulation step of every path that has one (K views per path of one
# fr_fisher_views call), then ONE fr_popgs_diag_criterion call that scores them and updates the paths' priors in place.

def popgs_round_schedule(path_lengths, acc_H_train_every):
    """The rounds of a batched evaluation.  Returns (order, rounds):
      order   the path indices by descending number of accumulation steps (stable), so that the paths active in a round are a
              prefix of it and a path's place in it is its row in the state tensor;
      rounds  rounds[m] = [(path, step, last), ...] in that order: the m-th accumulation step of every path that has one.
              `step` is 1-based, (step + 1) % acc_H_train_every == 0 (tester 2176); `last` marks a path's final accumulation
              step, whose estimate no later step reads."""
    acc = int(acc_H_train_every)
    if acc < 1:
        raise ValueError("acc_H_train_every must be >= 1")
    steps = [[s for s in range(1, int(n) + 1) if (s + 1) % acc == 0] for n in path_lengths]
    order = sorted(range(len(steps)), key=lambda i: -len(steps[i]))
    rounds = []
    for m in range(max((len(s) for s in steps), default=0)):
        rounds.append([(i, steps[i][m], len(steps[i]) == m + 1) for i in order if len(steps[i]) > m])
    return order, rounds


def popgs_path_value(point_terms, n_actions, final_EIG, path_end_weight=0.0, object_path_end_weight=0.0):
    """End of a path exactly as tester 2186-2191: the branch is chosen by `path_end_weight`, the final EIG is multiplied by
    `object_path_end_weight`.  `point_terms` are the (weighted) terms of the accumulation steps, added in order; a path without
    actions divides by 1 (the reference would divide by zero)."""
    total = 0.0
    for t in point_terms:
        total += float(t)
    n = max(int(n_actions), 1)
    final = float(final_EIG.item() if hasattr(final_EIG, "item") else final_EIG)
    if path_end_weight > 0:
        return total / n + float(object_path_end_weight) * final
    return (total + final) / n


def popgs_rows_from_flat(H_diag, P):
    """[means(3P) | opacity(P) | rot(4P) | scale(3P)] (gaussian_object.py:2100-2107, what compute_H_train_popgs returns)
    -> the scorer's row layout [P, 11] = [mean | opacity | scale | rot]."""
    h = H_diag.reshape(-1)
    if h.numel() != 11 * P:
        raise ValueError(f"H_train_diag has {h.numel()} entries, expected 11 * {P}")
    return torch.cat([h[:3 * P].reshape(P, 3), h[3 * P:4 * P].reshape(P, 1), h[8 * P:11 * P].reshape(P, 3),
                      h[4 * P:8 * P].reshape(P, 4)], dim=1).contiguous()


def evaluate_paths_popgs(slam, start_c2w, path_actions, final_EIGs, H_train_diag, *, criterion="topt", lam=1e-6, K=4,
                         forward_step_size=0.065, turn_angle=10., acc_H_train_every=5, path_point_weight=1.0,
                         path_end_weight=0.0, object_path_end_weight=0.0, cam_height=None, probes=None, chunk_bytes=4 << 30,
                         poses_w2c=None):
    """The list of total_path_EIG values of `path_evaluation_popgs` (tester 2121-2193), one per path.
    `slam`: a GaussianObjectSLAM with the grafted `_pose_probe_rows`; `H_train_diag`: what `compute_H_train_popgs` returns.
    `probes`: None draws the K upstream-gradient images of every accumulation step with torch.randn on the device; otherwise a
    callable probes(path_index, acc_index) -> [K, 3, H, W] (acc_index counts the path's accumulation steps from 0).  The
    reference's random stream (one draw per step, used or not) is not reproduced.
    Memory: one round holds paths x K x P x 44 bytes of probe rows (1.85 GB at 21 paths, K = 4, P = 500k; rounds beyond
    `chunk_bytes` are cut into several launches) beside the state, P x 44 bytes per path with two or more accumulation steps.
    poses_w2c: as in `evaluate_paths` -- the device poses [n_paths, Q, 4, 4] in place of the host roll-out and inversion."""
    from . import ops
    crit = str(criterion).lower()
    if crit not in ("topt", "dopt"):
        raise ValueError("criterion must be 'topt' or 'dopt'")
    K = int(K)
    start = np.array(start_c2w, dtype=np.float64, copy=True)
    if cam_height is not None:
        start[1, 3] = cam_height
    n_paths = len(path_actions)
    order, rounds = popgs_round_schedule([len(a) for a in path_actions], acc_H_train_every)
    place = {i: r for r, i in enumerate(order)}
    if poses_w2c is not None:
        poses_w2c = _check_poses_w2c(poses_w2c, path_actions, slam.params['means3D'].device)
    else:
        poses = [rollout(start, a, forward_step_size, turn_angle) for a in path_actions]
    point_terms = [[] for _ in range(n_paths)]
    if rounds:
        P = int(slam.params['means3D'].shape[0])
        dev = slam.params['means3D'].device
        prior0 = popgs_rows_from_flat(H_train_diag.detach().to(dev, torch.float32), P)
        # rows of the state: the paths that ever fold an estimate into their prior (a prefix of `order`)
        n_state = sum(1 for _, _, last in rounds[0] if not last)
        state = torch.empty((n_state, P, 11), dtype=torch.float32, device=dev)
        per = max(1, int(chunk_bytes // (K * P * 44)))
    for m, rnd in enumerate(rounds):
        cuts = sorted({0, len(rnd)} | set(range(per, len(rnd), per)) | ({n_state} if m == 0 and 0 < n_state < len(rnd) else set()))
        for v0, v1 in zip(cuts[:-1], cuts[1:]):
            part = rnd[v0:v1]
            assert all(place[i] == v0 + k for k, (i, _, _) in enumerate(part))
            if poses_w2c is not None:
                w2c = _gather_w2c(poses_w2c, [(i, s) for i, s, _ in part])
            else:
                c2w = np.stack([poses[i][s - 1] for i, s, _ in part])
                w2c = torch.from_numpy(np.linalg.inv(c2w)).float().to(dev)
            zs = None if probes is None else [z for i, _, _ in part for z in probes(i, m)]
            rows, vis = slam._pose_probe_rows(w2c, K, zs)
            writes = v1 <= n_state
            scores = ops.popgs_diag_criterion(
                rows, prior0 if m == 0 else state[v0:v1], lam, crit,
                prior_out=state[v0:v1] if writes else None,
                accumulate=torch.tensor([not last for _, _, last in part], dtype=torch.uint8) if writes else None,
                vis_count=vis.to(torch.int32).contiguous())
            del rows
            for (i, _, _), s in zip(part, scores.cpu().tolist()):            # the round's one host read
                point_terms[i].append(float(path_point_weight) * s)
    return [popgs_path_value(point_terms[i], len(path_actions[i]), final_EIGs[i], path_end_weight, object_path_end_weight)
            for i in range(n_paths)]
