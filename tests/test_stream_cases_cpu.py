"""The table of tests/stream_cases.py without a GPU: `real` and `decoy` of every case agree in names, shapes, dtypes and contiguity
(the stream-ordered run overwrites one with the other in place), every index input lies within its bounds (a wrong-stream bug must
show as a wrong number, never as an access out of bounds), and the two differ wherever the case does not keep them equal on
purpose."""
import numpy as np
import pytest

import stream_cases as sc


@pytest.fixture(scope="module", params=sc.names())
def pair(request):
    case = sc.by_name(request.param)
    return case, case.make(0), case.make(1)


def test_real_and_decoy_have_one_layout(pair):
    case, real, decoy = pair
    assert list(real) == list(decoy), case.name
    for k, r in real.items():
        d = decoy[k]
        assert isinstance(r, np.ndarray) and isinstance(d, np.ndarray), (case.name, k)
        assert r.shape == d.shape and r.dtype == d.dtype, (case.name, k, r.shape, d.shape, r.dtype, d.dtype)
        assert r.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"], (case.name, k)
        assert r.dtype in (np.float32, np.int32, np.int64, np.uint8), (case.name, k, r.dtype)
        if r.dtype == np.float32:
            assert np.isfinite(r).all() and np.isfinite(d).all(), (case.name, k)


def test_index_inputs_are_within_their_bounds(pair):
    case, real, decoy = pair
    integer = {k for k, v in real.items() if v.dtype in (np.int32, np.int64)}
    # every integer input is an index or a count the kernels act on: each needs a stated range (uint8 inputs are masks and flags)
    assert integer <= set(case.bounds), (case.name, integer - set(case.bounds))
    for k, (lo, hi) in case.bounds.items():
        for a in (real[k], decoy[k]):
            assert a.size and lo <= int(a.min()) and int(a.max()) < hi, (case.name, k, int(a.min()), int(a.max()), lo, hi)
    # a byte input is a mask or a flag, unless it has a stated range of its own (action codes) or the case names it as image bytes
    assert set(case.images) <= {k for k, v in real.items() if v.dtype == np.uint8}, (case.name, case.images)
    for k, v in real.items():
        if v.dtype == np.uint8 and k not in case.bounds and k not in case.images:
            assert int(v.max()) <= 1 and int(decoy[k].max()) <= 1, (case.name, k)


def test_real_and_decoy_differ(pair):
    case, real, decoy = pair
    assert set(case.same) <= set(real), (case.name, set(case.same) - set(real))
    varied = [k for k in real if k not in case.same]
    assert varied, case.name
    for k in varied:
        assert not np.array_equal(real[k], decoy[k]), f"{case.name}: {k} is the same in real and decoy"
    for k in case.same:
        assert np.array_equal(real[k], decoy[k]), f"{case.name}: {k} is listed as kept equal and differs"


def test_every_case_compares_something_and_names_its_rule():
    seen = set()
    for case in sc.cases():
        assert case.name not in seen
        seen.add(case.name)
        assert case.exact or case.close, case.name
        assert not (set(case.exact) & set(case.close)), case.name
        assert bool(case.close) == bool(case.close_from), f"{case.name}: a tolerance is quoted from an existing parity test, by name"
        assert case.sync_free or not case.repeat, f"{case.name}: a call that reads back inside cannot be made twice behind one blocker"
    assert sc.BLOCKER_MS >= 20.0 and sc.BLOCKER_MS <= sc.BLOCKER_CAP_MS == 250.0


# ---- the table is whole: every export that takes a stream is driven by some case -----------------------------------------------------------

# the exports that take NO stream, each by name: size and layout queries, house-keeping, the profiler switch, the planner's round cap
NO_STREAM = {
    "fr_version", "fr_last_error", "fr_build_id", "fr_init", "fr_profile_enable", "fr_profile_fetch", "fr_plan_round_cap",
    "fr_workspace_bytes", "fr_workspace_layout", "fr_fisher_workspace_bytes", "fr_fisher_workspace_layout", "fr_fisher_part_list_offset",
    "fr_backward_scratch_bytes", "fr_backward_pair_scratch_bytes",
    "fr_fisher_pose_workspace_bytes", "fr_fisher_pose_workspace_layout", "fr_render_views_workspace_bytes", "fr_render_views_workspace_layout",
    "fr_fisher_point_workspace_bytes", "fr_fisher_point_workspace_layout", "fr_popgs_diag_criterion_workspace_bytes",
    "fr_image_loss_workspace_bytes", "fr_frame_ingest_workspace_bytes", "fr_map_edit_workspace_bytes", "fr_rendervar_workspace_bytes",
    "fr_keyframe_valid_pixels_workspace_bytes", "fr_keyframe_overlap_workspace_bytes", "fr_knn_workspace_bytes", "fr_spatial_order_workspace_bytes",
    "fr_occ_workspace_bytes", "fr_plan_workspace_bytes", "fr_cloud_index_bytes", "fr_cloud_index_workspace_bytes", "fr_cloud_query_workspace_bytes",
    "fr_dbscan_workspace_bytes", "fr_target_select_workspace_bytes", "fr_view_metrics_workspace_bytes", "fr_loss_mask_workspace_bytes",
    "fr_bg_penalty_workspace_bytes", "fr_outside_mask_workspace_bytes",
}


def test_the_stream_taking_exports_are_the_ones_the_headers_say():
    from fisher_rast import _lib
    declared = sc.declared_exports()
    assert set(_lib.EXPORTS) == set(declared), set(_lib.EXPORTS) ^ set(declared)
    without = {n for n, params in declared.items() if "fr_stream_t" not in params}
    assert without == NO_STREAM, without ^ NO_STREAM                  # every name on the list, held against its declaration
    assert set(sc.stream_exports()) == set(_lib.EXPORTS) - NO_STREAM  # the recorder of the GPU test wraps exactly the others


def _uncovered(table):
    """the stream-taking exports that no case of `table` lists"""
    return set(sc.stream_exports()) - {n for case in table for n in case.covers}


def test_every_stream_taking_export_has_a_case():
    for case in sc.cases():
        assert case.covers, f"{case.name}: covers is empty"
        assert set(case.covers) <= set(sc.stream_exports()), (case.name, set(case.covers) - set(sc.stream_exports()))
    assert not _uncovered(sc.cases()), f"no stream-order case drives {sorted(_uncovered(sc.cases()))}"


# the exports that more than one case drives, with the number of cases; every other stream-taking export has exactly one
SHARED = {"fr_forward": 2, "fr_backward_ws": 3, "fr_fisher_views": 3, "fr_map_edit_apply": 2, "fr_map_edit_split_children": 2, "fr_occ_freespace": 5,
          "fr_occ_erode": 3, "fr_plan_grid": 3, "fr_plan_tiers": 3, "fr_plan_field": 3, "fr_plan_paths": 3, "fr_cloud_index_build": 2,
          "fr_cloud_query": 2, "fr_view_metrics": 2, "fr_view_metrics_summary": 2, "fr_loss_mask": 2, "fr_occ_grid_candidates": 2}


def test_no_covers_entry_can_go_unnoticed():
    """the number of cases behind every export is written down: taking any single entry out of any `covers` changes a count here, also
    where another case still drives the export (a new case for a listed export raises its number in this table)"""
    import collections
    from fisher_rast import _lib
    count = collections.Counter(n for case in sc.cases() for n in set(case.covers))
    assert all(len(set(case.covers)) == len(case.covers) for case in sc.cases())
    want = {n: SHARED.get(n, 1) for n in set(_lib.EXPORTS) - NO_STREAM}
    assert dict(count) == want, {n: (count.get(n, 0), want.get(n, 0)) for n in set(count) | set(want) if count.get(n, 0) != want.get(n, 0)}


def test_the_completeness_check_notices_a_missing_entry():
    """an export that only one case lists must be reported when that case leaves it out (the check is not vacuous); at the least the
    new units' entry points are such"""
    table = sc.cases()
    for name in ("fr_dbscan", "fr_target_select", "fr_rollout_actions", "fr_occ_frontiers", "fr_backward", "fr_outside_mask"):
        owners = [c for c in table if name in c.covers]
        assert len(owners) == 1, (name, [c.name for c in owners])
        thinned = [c._replace(covers=tuple(n for n in c.covers if n != name)) if c is owners[0] else c for c in table]
        assert _uncovered(thinned) == {name}


# ---- the scenes of the new cases have what the kernels' chains need ------------------------------------------------------------------------

def test_view_metrics_rows_of_real_and_decoy_are_far_apart():
    """one differing bit per output tensor is not enough: through the host harness over csrc/fr_eval_math.h, PSNR, SSIM, both depth
    errors and the three channel MSEs of every view -- and the summary's means -- differ between real and decoy by at least 1e-3 of
    their size (rounding is 1e-7), and the depth counts differ"""
    import eval_cases as ec
    h = ec.build_harness()
    f32, u8 = sc.by_name("view_metrics_f32_depth_mask"), sc.by_name("view_metrics_u8x4")
    runs = {}
    for which in (0, 1):
        a, b = f32.make(which), u8.make(which)
        runs["f32", which] = ec.harness_metrics(h, a["render"], a["gt_f32"], a["depth"], a["gt_depth"], a["mask"], valid_only=True)
        runs["u8", which] = ec.harness_metrics(h, b["render"], b["gt_u8x4"])

    def apart(x, y, what):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        assert np.isfinite(x).all() and np.isfinite(y).all(), what
        rel = np.abs(x - y) / np.maximum(np.abs(x), np.abs(y))
        assert (rel >= 1e-3).all(), (what, rel)
    for kind, columns in (("f32", [0, 1, 2, 3, 4, 5, 6]), ("u8", [0, 1, 4, 5, 6])):
        (rows, summary), (rows_d, summary_d) = runs[kind, 0], runs[kind, 1]
        apart(rows[:, columns], rows_d[:, columns], kind)
        apart(summary[1:3], summary_d[1:3], kind + " summary")
    assert (runs["f32", 0][0][:, 7] != runs["f32", 1][0][:, 7]).all()
    apart(runs["f32", 0][1][3:5], runs["f32", 1][1][3:5], "f32 summary of the depth errors")


def test_cluster_scenes_have_clusters_noise_and_a_long_band():
    import cluster_cases as cl
    for which in (0, 1):
        labels = cl.restate_dbscan(sc.by_name("dbscan_raw").make(which)["points"], cl.EPS, cl.MIN_SAMPLES)
        assert labels.max() >= 1 and (labels < 0).sum() >= 10, (which, labels.max(), (labels < 0).sum())
        d = sc.by_name("select_target").make(which)
        r = cl.restate_select(d["means3D"], d["scores"], sc.SELECT_BAND[0], sc.SELECT_BAND[1])
        # more than 256 rows in the band: the compaction's scan carries across rounds; clusters and noise among the rows above the threshold
        assert len(r["band_idx"]) > 256 and r["n_clusters"] >= 2 and (r["labels"] < 0).any() and r["max_label"] >= 0, \
            (which, len(r["band_idx"]), r["n_clusters"], r["max_label"])


def test_object_scene_has_cells_on_both_sides_of_the_rule():
    import goal_cases as gc
    import plan_cases as pc
    c = pc.make_case("door-3")
    for which in (0, 1):
        pts, want = sc.object_points(which)
        cells, counts = gc.np_object_cells(c["W"], c["H"], c["cell"], c["center"], pts, 3, c["W"] * c["H"])
        assert counts[0] == len(cells) > 256 and counts[1] == len(pts)
        assert sorted(map(tuple, cells.tolist())) == sorted(map(tuple, want.tolist()))
        assert len(want) < sc.OBJECT_BLOCK ** 2                      # some cells hold exactly 3: binned, and not "more than 3"


def test_action_poses_stand_on_their_cells():
    import action_cases as ac
    import plan_cases as pc
    c = pc.make_case("door-3")
    agent, goals = sc._action_poses(c, ac.yaw_pose)
    cell_of = lambda x, z: (int((z - c["center"][1]) / c["cell"] + c["H"] // 2), int((x - c["center"][0]) / c["cell"] + c["W"] // 2))
    assert cell_of(agent[0, 3], agent[2, 3]) == tuple(c["start"])
    assert [cell_of(float(g[0, 3]), float(g[2, 3])) for g in goals] == [tuple(g) for g in c["goals"]]
    assert pc.make_case("door-9")["goals"] == c["goals"] and pc.make_case("door-9")["start"] == c["start"]
