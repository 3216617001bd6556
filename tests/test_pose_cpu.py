"""CPU: the camera optimiser's host side and the reference side of its GPU tests -- the pose algebra against values recorded from the
reference's own functions (tests/golden/g19_pose.npz, oracle/gen_golden_pose.py), the ABI surface of the three new entry points, the class's
refusals, the groups table, the lr schedule and the checkpoint names."""
import ctypes
import os
import re

import pytest
import torch

from tests import pose_reference as PR
from tests.conftest import ROOT, load_golden

NEW_SYMBOLS = ("snerf_kplanes_gather_bwd_coords", "snerf_pose_apply", "snerf_raygen_pose_bwd")


def test_pose_algebra_matches_the_reference():
    g = load_golden("g19_pose")
    e = PR.pose_delta_transform(g["tangent"])
    # float64 against float64; the formula here (cross products, w w^T - |w|^2 I) rounds differently from the reference's matrix products:
    # a few ulp of entries of magnitude <= 1, and of translations of magnitude <= 4 in the composition
    torch.testing.assert_close(e, g["exp_map"], rtol=0, atol=1e-15)
    torch.testing.assert_close(PR.compose_poses(g["poses"], e), g["composed"], rtol=0, atol=4e-15)
    assert torch.equal(e[:8, :, :3], torch.eye(3, dtype=torch.float64).expand(8, 3, 3))  # zero row: the identity exactly
    assert torch.equal(PR.adjusted_c2w(g["poses"], g["tangent"]), PR.compose_poses(g["poses"], e))
    groups = torch.arange(64) % 7
    assert torch.equal(PR.adjusted_c2w(g["poses"], g["tangent"][:7], groups), PR.compose_poses(g["poses"], e[groups]))


def test_new_symbols_declared_exported_and_bound():
    from soccernerfs_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snerf.h")).read(), flags=re.S)
    l = _lib.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} is not declared in include/snerf.h"
        assert s in _lib.EXPORTS and hasattr(l, s)
        assert getattr(l, s).argtypes is not None, f"{s} has no ctypes argtypes"
    assert len(l.snerf_kplanes_gather_bwd_coords.argtypes) == 9 and len(l.snerf_pose_apply.argtypes) == 7
    assert l.snerf_abi_version() == 16 and l.snerf_abi_revision() == 2  # added to revision 2's surface, no new number
    # snerf_raygen_pose_bwd_args: 14 pointers, 6 int32
    assert ctypes.sizeof(_lib.RaygenPoseBwdArgs) == 14 * 8 + 6 * 4
    assert _lib.RaygenPoseBwdArgs.distortion_stride.offset == 14 * 8 and _lib.RaygenPoseBwdArgs.R.offset == 14 * 8 + 16


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument errors that are decided on the host.  Every call here passes NULL buffers or a size of zero (N = 0, M = 0, R = 0), for which no
    kernel can be launched whatever the order of the checks; the one non-NULL pointer is a host word that a size of zero never lets anyone read."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    d, c = _lib.KPlanesDesc(), _lib.Coords()
    d.n_scales, d.C, d.concat, d.n_coords = 1, 12, 0, 4
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 0, None, None, None, None, None) == -1
    assert b"C=12" in l.snerf_last_error()
    d.C = 8
    for k in range(4):
        d.res[0][k] = 4
    c.mode = 0
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 4, None, None, None, None, None) == -1
    assert b"pts is null" in l.snerf_last_error()
    word = (ctypes.c_float * 4)()
    ptr = ctypes.cast(word, ctypes.c_void_p)
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 0, None, None, ptr, None, None) == -1
    assert b"mode 1" in l.snerf_last_error()  # per-ray outputs need rays
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 0, None, None, None, None, None) == -1
    assert b"no output" in l.snerf_last_error()
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 0, None, ptr, None, None, None) == 0  # nothing to do
    c.mode = 2
    assert l.snerf_kplanes_gather_bwd_coords(ctypes.byref(d), None, ctypes.byref(c), 0, None, ptr, None, None, None) == -1
    assert l.snerf_pose_apply(None, None, None, 0, 2, None, None) == -1 and b"group" in l.snerf_last_error()
    assert l.snerf_pose_apply(None, None, None, 0, 0, None, None) == 0
    a = _lib.RaygenPoseBwdArgs()
    a.M, a.G, a.R = 5, 2, 0
    assert l.snerf_raygen_pose_bwd(ctypes.byref(a), None) == -1 and b"group" in l.snerf_last_error()
    a.G, a.distortion_stride = 5, 3
    assert l.snerf_raygen_pose_bwd(ctypes.byref(a), None) == -1 and b"distortion_stride" in l.snerf_last_error()
    a.distortion_stride = 0
    assert l.snerf_raygen_pose_bwd(ctypes.byref(a), None) == 0


def test_ray_gradients_refuses_what_it_does_not_cover(monkeypatch):
    """The refusals of KPlanesTrainConfig(ray_gradients=True) are decided before the trainer allocates anything, so they need no GPU: the
    view-dependent colour net and a process group of more than one rank."""
    from soccernerfs_amd.trainer import KPlanesTrainConfig, KPlanesTrainer

    with pytest.raises(NotImplementedError, match="disable_viewing_dependent=False"):
        KPlanesTrainer(KPlanesTrainConfig(ray_gradients=True, disable_viewing_dependent=False), 64, "cpu")
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda group=None: 0)
    with pytest.raises(NotImplementedError, match="world > 1"):
        KPlanesTrainer(KPlanesTrainConfig(ray_gradients=True), 64, "cpu", process_group=object())


def test_camera_optimizer_refusals_and_groups():
    from soccernerfs_amd.camera_optimizers import CameraOptimizer, CameraOptimizerConfig

    with pytest.raises(NotImplementedError, match="SE3"):
        CameraOptimizer(CameraOptimizerConfig(mode="SE3"), 4, "cpu")
    with pytest.raises(NotImplementedError, match="pose noise"):
        CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3", position_noise_std=0.1), 4, "cpu")
    with pytest.raises(ValueError, match="mode"):
        CameraOptimizer(CameraOptimizerConfig(mode="so3"), 4, "cpu")
    cfg = CameraOptimizerConfig(mode="SO3xR3")
    assert (cfg.lr, cfg.eps, cfg.max_steps, cfg.lr_final, cfg.param_group) == (6e-4, 1e-15, 10000, None, "camera_opt")
    assert tuple(CameraOptimizer(cfg, 4, "cpu").pose_adjustment.shape) == (4, 6)  # the reference's one row per image
    opt = CameraOptimizer(cfg, 5, "cpu", groups=torch.tensor([0, 1, 1, 2, 0]))
    assert tuple(opt.pose_adjustment.shape) == (3, 6) and opt.num_groups == 3 and float(opt.pose_adjustment.abs().max()) == 0.0
    for bad, msg in ((torch.tensor([0, 1, 1]), "expected an integer tensor"), (torch.tensor([0.0, 1, 1, 2, 0]), "expected an integer tensor"),
                     (torch.tensor([0, 1, 1, 3, 0]), "without gaps"), (torch.tensor([0, -1, 1, 2, 0]), "negative")):
        with pytest.raises(ValueError, match=msg):
            CameraOptimizer(cfg, 5, "cpu", groups=bad)
    off = CameraOptimizer(CameraOptimizerConfig(), 3, "cpu")
    assert not list(off.parameters()) and off.checkpoint_entries() == ({}, {})
    assert torch.equal(off(torch.tensor([0, 2])), torch.eye(4)[None, :3, :4].tile(2, 1, 1))


def test_pose_groups_from_camera_ids():
    from soccernerfs_amd.dataparsers import camera_pose_groups

    class T:
        ids = torch.tensor([12, 3, 12, 40, 3, 3], dtype=torch.uint8)

    assert camera_pose_groups(T()).tolist() == [1, 0, 1, 2, 0, 0]
    assert camera_pose_groups(T.ids).dtype == torch.int64
    with pytest.raises(ValueError, match="no camera ids"):
        camera_pose_groups(None)


def test_lr_schedule_matches_the_reference():
    from soccernerfs_amd.camera_optimizers import CameraOptimizer, CameraOptimizerConfig, exponential_decay_lr

    g = load_golden("g19_pose")
    steps = [int(s) for s in g["sched_steps"]]
    for name, lr_final in (("none", None), ("1e-5", 1e-5)):
        got = torch.tensor([exponential_decay_lr(s, 6e-4, lr_final, 10000) for s in steps], dtype=torch.float64)
        torch.testing.assert_close(got, g["sched_lr_" + name], rtol=1e-14, atol=0)
    opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 2, "cpu")
    assert opt.lr() == pytest.approx(6e-4, rel=1e-15) and opt.lr(9000) == pytest.approx(6e-4, rel=1e-15)  # lr_final None: constant


def test_checkpoint_names_round_trip(tmp_path):
    from soccernerfs_amd import checkpoint as CK
    from soccernerfs_amd.camera_optimizers import PIPELINE_KEY, CameraOptimizer, CameraOptimizerConfig

    assert PIPELINE_KEY == "datamanager.train_camera_optimizer.pose_adjustment"
    cfg = CameraOptimizerConfig(mode="SO3xR3")
    a = CameraOptimizer(cfg, 5, "cpu", groups=torch.tensor([0, 1, 1, 2, 0]))
    with torch.no_grad():
        a.pose_adjustment.copy_(torch.arange(18.0).reshape(3, 6) * 1e-3)
        a.exp_avg.fill_(0.25)
        a.exp_avg_sq.fill_(0.5)
    a.step_count = 7
    assert list(a.state_dict().keys()) == ["pose_adjustment"]
    pipe, opts = a.checkpoint_entries()
    assert list(pipe) == [PIPELINE_KEY] and list(opts) == ["camera_opt"]
    assert opts["camera_opt"]["param_groups"][0]["eps"] == 1e-15 and float(opts["camera_opt"]["state"][0]["step"]) == 7.0
    model = torch.nn.Module()
    model.field = torch.nn.Module()
    model.field.w = torch.nn.Parameter(torch.ones(3))
    CK.save_checkpoint(str(tmp_path / "on"), 6, model, dict(opts), extra_pipeline=pipe)
    CK.save_checkpoint(str(tmp_path / "off"), 6, model, {})
    on = torch.load(CK.checkpoint_path(str(tmp_path / "on"), 6), weights_only=False)
    off = torch.load(CK.checkpoint_path(str(tmp_path / "off"), 6), weights_only=False)
    assert set(on["pipeline"]) - set(off["pipeline"]) == {PIPELINE_KEY} and list(off["pipeline"]) == ["_model.field.w"] and off["optimizers"] == {}
    b = CameraOptimizer(cfg, 5, "cpu", groups=torch.tensor([0, 1, 1, 2, 0]))
    assert CK.load_checkpoint(str(tmp_path / "on"), model, camera_optimizer=b)[0] == 7
    assert torch.equal(b.pose_adjustment, a.pose_adjustment) and torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    assert b.step_count == 7
    with torch.no_grad():
        b.pose_adjustment.fill_(1.0)
    CK.load_checkpoint(str(tmp_path / "off"), model, camera_optimizer=b)  # a file written with the feature off: start from zeros
    assert float(b.pose_adjustment.abs().max()) == 0.0 and float(b.exp_avg.abs().max()) == 0.0 and b.step_count == 0
    with pytest.raises(RuntimeError, match="the checkpoint holds"):
        CK.load_checkpoint(str(tmp_path / "on"), model, camera_optimizer=CameraOptimizer(cfg, 5, "cpu"))


def test_excluded_share_of_the_coordinate_cases_is_below_one_percent():
    """The GPU test skips samples within 1e-4 texel of a lattice line; for the committed seeds that is < 1 % of every case."""
    for c in PR.COORDS_CASES:
        d = PR.make_coords_case(c)
        assert 1.0 - float(PR.comparable_samples(c, d).double().mean()) < 0.01, PR.case_id(c)


def test_deviation_record_covers_every_case():
    b = PR.load_bounds()
    assert b["factor"] == PR.FACTOR
    assert sorted(b["coords"]) == sorted(PR.case_id(c) for c in PR.COORDS_CASES)
    for c in PR.COORDS_CASES:
        assert b["coords"][PR.case_id(c)]["seed"] == c["seed"]
    keys = [f"{k}-{g}-{a}_clamp" for k in PR.POSE_TABLES for g in PR.POSE_GROUPS for a in ("below", "above")]
    assert sorted(b["pose_bwd"]) == sorted(keys) and sorted(b["pose_apply"]) == sorted(keys)
    assert all(f"step{i}" in b["three_steps"] for i in (1, 2, 3))


def test_trainer_config_has_the_switch_off_by_default():
    from soccernerfs_amd.trainer import KPlanesTrainConfig

    assert KPlanesTrainConfig().ray_gradients is False
