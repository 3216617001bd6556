"""ctypes binding of libsnerf.so (C ABI: include/snerf.h).  The product path has NO fallback:
if the HIP library is missing or stale the import fails loudly."""
import ctypes as C
import os

import torch  # noqa: F401  -- FIRST: libsnerf must bind to the HIP runtime torch already loaded (same SONAME)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libsnerf.so")

MAX_SCALES = 8
ABI_VERSION = 16
ABI_REVISION = 2  # additions on top of ABI 16 (include/snerf.h: SNERF_ABI_REVISION)


class KPlanesDesc(C.Structure):
    _c_struct_ = "snerf_kplanes_desc"
    _fields_ = [
        ("n_scales", C.c_int32),
        ("C", C.c_int32),
        ("concat", C.c_int32),
        ("n_coords", C.c_int32),
        ("res", (C.c_int32 * 4) * MAX_SCALES),
        ("off", (C.c_int64 * 6) * MAX_SCALES),
    ]


class Coords(C.Structure):
    _c_struct_ = "snerf_coords"
    _fields_ = [
        ("mode", C.c_int32),
        ("S", C.c_int32),
        ("rescale", C.c_int32),
        ("contract", C.c_int32),
        ("pts", C.c_void_p),
        ("origins", C.c_void_p),
        ("dirs", C.c_void_p),
        ("times", C.c_void_p),
        ("ebins", C.c_void_p),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
    ]


class ResampleArgs(C.Structure):
    _c_struct_ = "snerf_resample_args"
    _fields_ = [
        ("density", C.c_void_p), ("weights_in", C.c_void_p), ("ebins_prev", C.c_void_p), ("weights_out", C.c_void_p),
        ("sbins_prev", C.c_void_p), ("u_or_rand", C.c_void_p), ("nears", C.c_void_p), ("fars", C.c_void_p),
        ("sbins_out", C.c_void_p), ("ebins_out", C.c_void_p), ("inds_out", C.c_void_p),
        ("R", C.c_int32), ("S_prev", C.c_int32), ("S", C.c_int32),
        ("u_mode", C.c_int32), ("rand_cols", C.c_int32), ("kind", C.c_int32),
        ("anneal", C.c_float), ("histogram_padding", C.c_float), ("eps", C.c_float),
    ]


class MlpDesc(C.Structure):
    _c_struct_ = "snerf_mlp_desc"
    _fields_ = [("d_in", C.c_int32), ("hidden", C.c_int32), ("n_hidden", C.c_int32), ("d_out", C.c_int32),
                ("hidden_act", C.c_int32), ("out_act", C.c_int32), ("operands", C.c_int32)]


class DensityBwdLevel(C.Structure):
    """snerf_density_bwd_level: one proposal level of snerf_kplanes_density_bwd (pointers to its descriptors and buffers)."""
    _c_struct_ = "snerf_density_bwd_level"
    _fields_ = [("desc", C.c_void_p), ("planes", C.c_void_p), ("coords", C.c_void_p), ("N", C.c_int64), ("net", C.c_void_p), ("W", C.c_void_p),
                ("gdens", C.c_void_p), ("grad_planes", C.c_void_p), ("workspace", C.c_void_p), ("gX", C.c_void_p)]


class AdamDyn(C.Structure):
    """snerf_adam_dyn: device-resident optimiser state of one parameter group (8 x 4 bytes; lives in a torch int32[8] tensor)."""
    _c_struct_ = "snerf_adam_dyn"
    _fields_ = [("nonfinite", C.c_int32), ("t", C.c_int32), ("skipped", C.c_int32), ("dropped", C.c_int32),
                ("step_size", C.c_float), ("inv_sqrt_bc2", C.c_float), ("skip", C.c_int32), ("_pad", C.c_int32)]


class RenderArgs(C.Structure):
    _c_struct_ = "snerf_render_args"
    _fields_ = [("weights", C.c_void_p), ("rgb", C.c_void_p), ("ebins", C.c_void_p), ("bg", C.c_void_p),
                ("R", C.c_int32), ("S", C.c_int32), ("bg_mode", C.c_int32), ("training", C.c_int32),
                ("rgb_out", C.c_void_p), ("acc_out", C.c_void_p), ("depth_median", C.c_void_p), ("depth_expected", C.c_void_p),
                ("median_rgb", C.c_void_p), ("median_index", C.c_void_p)]


class RayTrainArgs(C.Structure):
    _c_struct_ = "snerf_ray_train_args"
    _fields_ = [("density", C.c_void_p), ("ebins", C.c_void_p), ("sbins", C.c_void_p), ("rgb", C.c_void_p), ("bg", C.c_void_p), ("target", C.c_void_p),
                ("R", C.c_int32), ("S", C.c_int32), ("bg_mode", C.c_int32), ("go_scale", C.c_float), ("dist_scale", C.c_float),
                ("weights", C.c_void_p), ("rgb_out", C.c_void_p), ("acc_out", C.c_void_p), ("depth_median", C.c_void_p), ("sqerr_rays", C.c_void_p),
                ("dist_rays", C.c_void_p), ("g_rgb", C.c_void_p), ("g_density", C.c_void_p), ("g_weights", C.c_void_p), ("nonfinite_flag", C.c_void_p)]


class RaygenArgs(C.Structure):
    _c_struct_ = "snerf_raygen_args"
    _fields_ = [("indices", C.c_void_p), ("fx", C.c_void_p), ("fy", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p),
                ("c2w", C.c_void_p), ("cam_times", C.c_void_p),
                ("R", C.c_int32), ("collide", C.c_int32), ("training", C.c_int32), ("near_plane", C.c_float),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("origins", C.c_void_p), ("dirs", C.c_void_p), ("pixel_area", C.c_void_p), ("dir_norm", C.c_void_p),
                ("times", C.c_void_p), ("nears", C.c_void_p), ("fars", C.c_void_p)]


class RaygenFrameArgs(C.Structure):
    """snerf_raygen_frame_args (ABI 16 revision 1, csrc/render_eval.hip): the rays of pixels [p0, p1) of one camera."""
    _c_struct_ = "snerf_raygen_frame_args"
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("c2w", C.c_float * 12), ("time", C.c_float),
                ("W", C.c_int32), ("H", C.c_int32), ("_pad", C.c_int32), ("p0", C.c_int64), ("p1", C.c_int64),
                ("near_plane", C.c_float), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
                ("origins", C.c_void_p), ("dirs", C.c_void_p), ("pixel_area", C.c_void_p), ("dir_norm", C.c_void_p),
                ("times", C.c_void_p), ("nears", C.c_void_p), ("fars", C.c_void_p)]


class RaygenLensArgs(C.Structure):
    """snerf_raygen_lens_args (ABI 16 revision 2, csrc/raygen.hip): RaygenArgs' fields, then the distortion table and its stride (6 or 0)."""
    _c_struct_ = "snerf_raygen_lens_args"
    _fields_ = RaygenArgs._fields_ + [("distortion", C.c_void_p), ("distortion_stride", C.c_int32)]


class RaygenFrameLensArgs(C.Structure):
    """snerf_raygen_frame_lens_args (ABI 16 revision 2, csrc/render_eval.hip): RaygenFrameArgs' fields, then the camera's k1 k2 k3 k4 p1 p2."""
    _c_struct_ = "snerf_raygen_frame_lens_args"
    _fields_ = RaygenFrameArgs._fields_ + [("distortion", C.c_float * 6)]


class RaygenCamArgs(C.Structure):
    """snerf_raygen_cam_args (added to ABI 16 revision 2, csrc/raygen.hip): RaygenLensArgs' fields, then the camera-type table and its stride
    (1: int32 [M], 0: one shared value); distortion and camera_type may be null."""
    _c_struct_ = "snerf_raygen_cam_args"
    _fields_ = RaygenLensArgs._fields_ + [("camera_type", C.c_void_p), ("camera_type_stride", C.c_int32)]


class RaygenFrameCamArgs(C.Structure):
    """snerf_raygen_frame_cam_args (added to ABI 16 revision 2, csrc/render_eval.hip): RaygenFrameLensArgs' fields, then the camera's type (1..3)
    and whether the distortion row is a lens (0: it is not read)."""
    _c_struct_ = "snerf_raygen_frame_cam_args"
    _fields_ = RaygenFrameLensArgs._fields_ + [("camera_type", C.c_int32), ("has_distortion", C.c_int32)]


class RaygenPoseBwdArgs(C.Structure):
    """snerf_raygen_pose_bwd_args (added to ABI 16 revision 2, csrc/raygen.hip): the batch, the camera table, the pose rows and the ray gradients."""
    _c_struct_ = "snerf_raygen_pose_bwd_args"
    _fields_ = [("indices", C.c_void_p), ("fx", C.c_void_p), ("fy", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p), ("c2w", C.c_void_p),
                ("distortion", C.c_void_p), ("camera_type", C.c_void_p), ("pose_adjustment", C.c_void_p), ("group", C.c_void_p),
                ("g_origins", C.c_void_p), ("g_dirs", C.c_void_p), ("grad_pose_fx", C.c_void_p), ("nonfinite_flag", C.c_void_p),
                ("distortion_stride", C.c_int32), ("camera_type_stride", C.c_int32), ("M", C.c_int32), ("G", C.c_int32), ("R", C.c_int32),
                ("_pad", C.c_int32)]


class TgridDesc(C.Structure):
    _c_struct_ = "snerf_tgrid_desc"
    _fields_ = [("D", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("grid_C", C.c_int32), ("H", C.c_int32), ("gridtype", C.c_int32),
                ("align_corners", C.c_int32), ("S", C.c_float), ("offsets", C.c_int32 * 33)]


class TgridTilePlan(C.Structure):
    """snerf_tgrid_tile_plan (ABI 14): the tiling of a temporal-grid table for the owner-computes backward (csrc/tgrid_tiles.hip)."""
    _c_struct_ = "snerf_tgrid_tile_plan"
    _fields_ = [("tile_rows_log2", C.c_int32), ("n_tiles", C.c_int32), ("n_chunks", C.c_int32), ("chunk", C.c_int32), ("first_tiled_level", C.c_int32),
                ("lds_bytes", C.c_int32), ("tile_start", C.c_int32 * 33), ("_pad", C.c_int32), ("count_ints", C.c_int64), ("record_capacity", C.c_int64)]


class HashgridTilePlan(C.Structure):
    """snerf_hashgrid_tile_plan (ABI 14, csrc/hashgrid_tiles.hip)."""
    _c_struct_ = "snerf_hashgrid_tile_plan"
    _fields_ = [("tile_rows_log2", C.c_int32), ("n_tiles", C.c_int32), ("n_chunks", C.c_int32), ("chunk", C.c_int32), ("lds_bytes", C.c_int32), ("first_tiled_level", C.c_int32),
                ("tile_start", C.c_int32 * 33), ("_pad2", C.c_int32), ("count_ints", C.c_int64), ("record_capacity", C.c_int64)]


class HashgridDesc(C.Structure):
    _c_struct_ = "snerf_hashgrid_desc"
    _fields_ = [("D", C.c_int32), ("F", C.c_int32), ("L", C.c_int32), ("scale", C.c_float * 32), ("resolution", C.c_int32 * 32),
                ("offsets", C.c_int32 * 33)]


# Every entry point include/snerf.h declares, one line each: "<return>:<parameters in order>".  A new entry point is two edits, the header and
# its line here; tests/test_binding_cpu.py parses the header and fails until the two agree.
#   parameters  P pointer (any T*, snerf_stream_t)   I int32_t / int   L int64_t   F float
#   return      s status int (0, or an error code for check)   i value int   l int64_t   z const char*
SIGNATURES = {
    "snerf_abi_version": "i:",
    "snerf_abi_revision": "i:",
    "snerf_last_error": "z:",
    "snerf_target_arch": "z:",
    "snerf_kplanes_gather_fwd": "s:PPPLPP",
    "snerf_kplanes_gather_bwd": "s:PPPLPPP",
    "snerf_kplanes_gather_bwd_coords": "s:PPPLPPPPP",
    "snerf_kplanes_gather_bwd_fx": "s:PPPLPPP",
    "snerf_fx_to_float": "s:PPLIP",
    "snerf_spaced_bins": "s:PPPIIIIPPP",
    "snerf_weights_fwd": "s:PPIIPP",
    "snerf_weights_bwd": "s:PPPIIPIPP",
    "snerf_pdf_resample": "s:PP",
    "snerf_mlp_param_count": "l:P",
    "snerf_mlp_supported": "i:P",
    "snerf_dense_fwd": "s:PIIIPILPIP",
    "snerf_dense_bwd": "s:PIIIPILPIPIPIPP",
    "snerf_dense_lp_supported": "i:III",
    "snerf_dense_fwd_lp": "s:PIIIPILPIIP",
    "snerf_dense_bwd_lp": "s:PIIIPILPIPIPIPPIP",
    "snerf_dense_bwd_fx": "s:PIIIPILPIPIPIPP",
    "snerf_mlp_fwd": "s:PPPILPIIPP",
    "snerf_mlp_bwd": "s:PPPILPIIPPIPP",
    "snerf_mlp_bwd_tile": "s:PPPILPIIPPIPP",
    "snerf_mlp_gw_workspace_floats": "l:P",
    "snerf_mlp_bwd_ws": "s:PPPILPIIPPIPP",
    "snerf_mlp_gw_reduce": "s:PPPP",
    "snerf_mlp_bwd_x16": "s:PPPILPIIPPIPP",
    "snerf_mlp_bwd_x16_quotient_ws": "s:PPPILPIIPPIPIPPPP",
    "snerf_mlp_bwd_x16_quotient": "s:PPPILPIIPPIPIPPPP",
    "snerf_mlp_bwd_fx": "s:PPPILPIIPPIPP",
    "snerf_kplanes_field_fwd_supported": "i:PPP",
    "snerf_kplanes_field_fwd": "s:PPPLPPPPPPPPPP",
    "snerf_kplanes_field_fwd_ordered": "s:PPPLPPPPPPPPPPP",
    "snerf_kplanes_field_render_supported": "i:PPPI",
    "snerf_kplanes_field_render": "s:PPPIPPPPFPPPPPPP",
    "snerf_kplanes_color_input_fwd": "s:PIPLPP",
    "snerf_kplanes_color_input_bwd": "s:PILPP",
    "snerf_kplanes_color_bwd_vd_supported": "i:P",
    "snerf_kplanes_color_bwd_vd": "s:PPPIPLPIPPP",
    "snerf_kplanes_color_bwd_vd_ws": "s:PPPIPLPIPPP",
    "snerf_kplanes_density_fwd_supported": "i:PP",
    "snerf_kplanes_density_fwd": "s:PPPLPPPPP",
    "snerf_kplanes_density_bwd_supported": "i:PP",
    "snerf_kplanes_density_bwd": "s:PIP",
    "snerf_kplanes_density_bwd_budget": "s:PIIP",
    "snerf_render_fwd": "s:PP",
    "snerf_ray_train_fwd_bwd": "s:PP",
    "snerf_render_bwd": "s:PPPIPPIIPPIP",
    "snerf_render_mse_bwd": "s:PPPIPPFIIPPPP",
    "snerf_distortion": "s:PPIIFPPIP",
    "snerf_interlevel": "s:PPIPPIIFPPP",
    "snerf_depth_loss": "s:PPPPFIIFPPIP",
    "snerf_urf_depth_loss": "s:PPPPPFIIFPPPIP",
    "snerf_plane_reg": "s:PPPFFFPIIP",
    "snerf_adam_prepare": "s:PFFFIIP",
    "snerf_adam_step": "s:PPPPPLFFFFIFIPP",
    "snerf_adam_planes_step": "s:PPPPPPFFFPIFFFFIFIPP",
    "snerf_adam_planes_step_range": "s:PPPPPPFFFPIFFFFIFILLPP",
    "snerf_comm_unique_id": "s:P",
    "snerf_comm_create": "s:IIPP",
    "snerf_comm_destroy": "s:P",
    "snerf_allreduce_grads": "s:PPLP",
    "snerf_raygen": "s:PP",
    "snerf_raygen_frame": "s:PP",
    "snerf_raygen_lens": "s:PP",
    "snerf_raygen_frame_lens": "s:PP",
    "snerf_raygen_cam": "s:PP",
    "snerf_raygen_frame_cam": "s:PP",
    "snerf_pose_apply": "s:PPPIIPP",
    "snerf_raygen_pose_bwd": "s:PP",
    "snerf_sample_pixels_uniform": "s:PIIIIPPPP",
    "snerf_sample_pixels_sphere": "s:PIIIIPPPP",
    "snerf_mask_pack": "s:PLLLPPP",
    "snerf_sample_pixels_masked": "s:PIIIIPPLPPPP",
    "snerf_sort_rays_by_key": "s:PPIIPIPPP",
    "snerf_ray_time_order": "s:PIPP",
    "snerf_aabb_collide": "s:PPIPFIPPP",
    "snerf_tgrid_encode_fwd": "s:PPPPPILPP",
    "snerf_tgrid_encode_fwd_dydx": "s:PPPPPILPPP",
    "snerf_tgrid_input_bwd": "s:PPLIIIPP",
    "snerf_tgrid_encode_bwd": "s:PPPPILPPP",
    "snerf_tgrid_encode_bwd_fx": "s:PPPPILPPP",
    "snerf_tgrid_density_fwd_supported": "i:PP",
    "snerf_tgrid_density_fwd": "s:PPPPILPPPP",
    "snerf_tgrid_tile_plan_make": "s:PLIIP",
    "snerf_tgrid_bwd_bin": "s:PPPPILPPPPPP",
    "snerf_tgrid_bwd_tiles": "s:PPLPPPPPP",
    "snerf_tgrid_bwd_tiles_adam": "s:PPLPPPPPPPPFFFFIIIPP",
    "snerf_tgrid_encode_bwd_levels": "s:PPPPILPPIIP",
    "snerf_tgrid_tv_fwd": "s:PLIIIPIP",
    "snerf_tgrid_tv_bwd": "s:PLIIIPPP",
    "snerf_tgrid_tv_fwd_bwd": "s:PLIIIFPIPP",
    "snerf_tgrid_tv_sign": "s:PLIIIFPIPP",
    "snerf_adam_step_tv": "s:PPPPLIIIPFFFFIFIPP",
    "snerf_hashgrid_layout": "l:PIFI",
    "snerf_hashgrid_encode_fwd": "s:PPPLPP",
    "snerf_hashgrid_encode_bwd": "s:PPPLPPPP",
    "snerf_hashgrid_encode_bwd_fx": "s:PPPLPPPP",
    "snerf_hashgrid_tile_plan_make": "s:PLIIP",
    "snerf_hashgrid_encode_bwd_levels": "s:PPPLPPPIIP",
    "snerf_hashgrid_bwd_bin": "s:PPPLPPPPP",
    "snerf_hashgrid_bwd_tiles": "s:PPPLPPPPP",
    "snerf_hashgrid_bwd_tiles_adam": "s:PPPLPPPPPPPFFFFIP",
    "snerf_nerfplayer_mix_fwd": "s:PPPPLIPPP",
    "snerf_nerfplayer_mix_bwd": "s:PPPPPPLIPPPPP",
    "snerf_nerfacto_head_input_fwd": "s:PPPPILPP",
    "snerf_nerfacto_head_input_bwd": "s:PPILPPPP",
    "snerf_trunc_exp_fwd": "s:PLPP",
    "snerf_trunc_exp_bwd": "s:PPLPP",
    "snerf_basis_rgb_fwd": "s:PIPLIPP",
    "snerf_basis_rgb_bwd": "s:PIPPPLIPPP",
    "snerf_ist_maps": "s:PIIIIPPFPP",
    "snerf_isg_maps": "s:PIIIIIPPPIFPPP",
    "snerf_ist_sample": "s:PIIPPIPIPP",
    "snerf_kplanes_sort_workspace": "s:PLPP",
    "snerf_kplanes_sort_samples": "s:PPLPPPP",
    "snerf_kplanes_gradvec": "s:PPPLPPIP",
    "snerf_kplanes_scatter_sorted": "s:PLPIPPP",
    "snerf_kplanes_quotient_supported": "i:PL",
    "snerf_kplanes_quotient_prepare": "s:PLPPPPIPPP",
    "snerf_kplanes_scatter_quotient_scales": "s:PPLPPPIIP",
    "snerf_kplanes_quotient_fixup": "s:PPPLPPIPIIPP",
    "snerf_kplanes_scatter_sorted_scales": "s:PLPIPPIIP",
}
EXPORTS = list(SIGNATURES)

_ARG = {"P": C.c_void_p, "I": C.c_int32, "L": C.c_int64, "F": C.c_float}
_RET = {"s": C.c_int, "i": C.c_int, "l": C.c_int64, "z": C.c_char_p}


def _declare(fn, signature: str):
    fn.restype = _RET[signature[0]]
    fn.argtypes = [_ARG[k] for k in signature[2:]]


def bind(path: str):
    """Loads the library at `path` and declares every entry of SIGNATURES on it; one that lacks any of them, or is of another ABI, is refused."""
    l = C.CDLL(path)
    missing = [s for s in SIGNATURES if not hasattr(l, s)]
    if missing:  # a library from before an entry was added must fail here, not at the first call
        some = ", ".join(missing[:8]) + (f", ... ({len(missing)} in all)" if len(missing) > 8 else "")
        raise RuntimeError(f"libsnerf at {path} lacks {some} (ABI {ABI_VERSION} revision {ABI_REVISION}): rebuild the library")
    for name, signature in SIGNATURES.items():
        _declare(getattr(l, name), signature)
    if l.snerf_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libsnerf ABI {l.snerf_abi_version()} != binding {ABI_VERSION}: rebuild the library")
    if l.snerf_abi_revision() != ABI_REVISION:
        raise RuntimeError(f"libsnerf ABI {ABI_VERSION} revision {l.snerf_abi_revision()} != binding revision {ABI_REVISION}: rebuild the library")
    # snerf_coords.contract took the struct's padding slot without a new symbol or revision: a library from before it would load and IGNORE the
    # field.  One host-side call tells them apart -- this header's library refuses contract = 2 before it looks at anything else that is empty
    # here (N = 0: nothing is launched either way), an older one returns success.
    desc, coords = KPlanesDesc(), Coords()
    desc.n_scales, desc.C, desc.n_coords = 1, 8, 3
    for k in range(3):
        desc.res[0][k] = 1
    coords.mode, coords.S, coords.contract = 1, 1, 2
    if l.snerf_kplanes_gather_fwd(C.byref(desc), None, C.byref(coords), 0, None, None) == 0:
        raise RuntimeError(f"libsnerf at {path} predates snerf_coords.contract (it accepts contract = 2): rebuild the library")
    return l


_lib = None
entries = {}  # "kplanes_gather_fwd" -> the loaded library's snerf_kplanes_gather_fwd: what call() looks a launch up in (filled by lib())


def lib():
    """Returns the loaded library, raising a RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP library is the product path and has no fallback. "
                "Build it with `python -m soccernerfs_amd.build` (or __graft_entry__.build())."
            )
        _lib = bind(LIB_PATH)
        entries.update((name[len("snerf_"):], getattr(_lib, name)) for name in SIGNATURES)
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().snerf_last_error().decode()
        raise RuntimeError(f"libsnerf {what} failed (code {rc}): {msg}")


def call(name: str, *args):
    """Launches snerf_<name>(*args) and raises on a non-zero code, under the entry's own name."""
    if not entries:
        lib()
    check(entries[name](*args), name)
