"""Every launching ABI entry under guard (tests/_abi_guard.py), at small ragged
shapes.  No new references: each case runs a check body the suite already has
inside `guarded_abi()`, so its float64 / golden assertions also prove that
relocating the buffers changed nothing, while the harness asserts that no
launch writes outside a buffer and that two runs from poisoned outputs and
scratch agree byte for byte.  Each family declares the entries it must hit.

Adding a case for a new entry: append a row to FAMILIES naming an existing
check of the entry's own test file, its arguments at the smallest ragged shape
the entry supports -- one per kernel variant its dispatcher can pick -- the
entry itself, and the `*_supported` query that must accept those shapes."""
import importlib
import inspect

import pytest
import torch

from tests._abi_guard import guarded_abi
from tests.golden.make_golden import NEAREST_CASES, NEWCRF_CASES, RESIZE_CASES, SAM_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    import monocular_depth_estimation_amd  # noqa: F401  (loads libmde_hip.so, raises if absent)


def _k(names, rows):
    names = names.split(",")
    return [dict(zip(names, r if len(names) > 1 else (r,))) for r in rows]


_BF = ("mde_bilinear_fwd", "mde_bilinear_bwd")
_C3 = ("mde_conv3x3_fwd", "mde_conv3x3_bwd_data", "mde_conv3x3_wgrad")

_PW = [(16, 8), (16, 16), (32, 16), (32, 32), (64, 32), (32, 64), (16, 32), (64, 64)]


# the *_supported (or workspace) query a family's shapes must satisfy, from its arguments
def _WINO_OK(k):
    return "mde_wino_supported", (k["cin"], k["cout"], k["h"], k["w"], 0)


def _PW_OK(k):
    return "mde_pointwise_supported", (k["cin"], k["cout"], k["h"], k["w"])


def _C3W_OK(k):
    return "mde_conv3x3_wgrad_workspace", (k["n"], k["cin"], k["cout"], k["h"], k["w"], 0)


def _S2W_OK(k):
    return "mde_conv3x3s2_wgrad_workspace", (k["n"], k["cin"], k["cout"], k["h"], k["w"], 0)


def _C1_OK(k):
    return "mde_conv1x1_supported", (k["cin"], k["cout"], k["h"], k["w"], k["stride"], 0)


# (test module, check, [arguments ...], entries every one of these runs must hit
#  [, the query that must accept the shape])
FAMILIES = [
    # ------------------------------------------------------------------ resize
    ("test_gpu_parity", "test_bilinear_full_size_adjoint_and_oracle_rows", _k("shape,kw", [
        ((3, 5, 3, 6), dict(scale_factor=2)), ((2, 3, 11, 7), dict(scale_factor=2)),
        ((2, 4, 9, 130), dict(scale_factor=2)), ((1, 2, 5, 3), dict(scale_factor=4)),
        ((2, 3, 9, 70), dict(scale_factor=4)), ((2, 2, 7, 66), dict(scale_factor=8)),
        ((2, 64, 2, 3), dict(size=(8, 12))), ((2, 3, 100, 150), dict(size=(310, 470))),
        ((1, 2, 10, 10), dict(size=(200, 210))),
        ((2, 3, 37, 41), dict(size=(111, 90), align_corners=True))]), _BF),
    ("test_gpu_parity", "test_bilinear_golden", _k("case", RESIZE_CASES), _BF),
    ("test_gpu_parity", "test_nearest_golden_bit_exact", _k("case", NEAREST_CASES),
     ("mde_nearest_fwd", "mde_nearest_bwd")),
    ("test_gpu_parity", "test_nearest_pyramid_matches_two_nearest_calls",
     _k("n,c,h,w", [(2, 3, 8, 16), (3, 2, 12, 40)]),
     ("mde_nearest_pyramid", "mde_nearest_fwd", "mde_nearest_bwd")),
    ("test_gpu_parity", "test_nearest_pyramid_matches_two_nearest_calls",   # h % 4: not fused
     _k("n,c,h,w", [(2, 3, 10, 20)]), ("mde_nearest_fwd", "mde_nearest_bwd")),
    ("test_gpu_se_bn", "test_grad_slot_bilinear_two_consumers", _k("n,c,h,w", [(3, 32, 12, 20)]),
     ("mde_bilinear_bwd2",)),
    # ------------------------------------------------- skip / pointwise / SE
    ("test_gpu_parity", "test_skip_reduce_vs_oracle", _k("n,cin,cout,h,w", [
        (2, 8, 4, 9, 11), (2, 40, 24, 7, 13), (2, 64, 32, 10, 10), (2, 16, 1, 48, 64)]),
     ("mde_skip_reduce_fwd", "mde_skip_reduce_bwd")),
    ("test_gpu_parity", "test_se_cat_vs_oracle", _k("n,ca,cb,h,w", [(2, 8, 8, 30, 41)]),
     ("mde_se_fwd", "mde_se_bwd")),
    ("test_gpu_parity", "test_se_golden", _k("tag,ch,red", [("se16", 16, 1), ("se32r4", 32, 4)]),
     ("mde_se_fwd", "mde_se_bwd")),
    ("test_gpu_se_bn", "test_se_bn_cat_vs_float64", _k("n,ca,cb,h,w,offset", [
        (3, 16, 16, 13, 18, 0.0), (4, 4, 12, 1, 1, 0.0)]), ("mde_se_bn_fwd", "mde_se_bn_bwd")),
    ("test_gpu_se_bn", "test_skip_reduce_bn_vs_float64", _k("n,cin,cout,h,w", [
        (3, 4, 1, 10, 14), (2, 64, 32, 12, 16)]),
     ("mde_skip_reduce_bn_fwd", "mde_skip_reduce_bn_bwd")),
    ("test_gpu_mobilenet", "test_se_hardsigmoid_vs_torch", _k("n,c,cr,h,w", [(3, 120, 32, 7, 5)]),
     ("mde_se_gate_fwd", "mde_se_gate_bwd")),
    # ---------------------------------------------- pointwise, fused branches
    ("test_gpu_conv3x3", "test_fused_bn_relu_pointwise_branch_vs_float64",
     _k("cin,e,eo,h,w,train", [(3, 32, 16, 16, 48, True)]),
     ("mde_conv3x3_fwd_stats", "mde_batchnorm_fwd_coef_stats", "mde_pointwise_fwd_stats",
      "mde_batchnorm_fwd_train_stats", "mde_batchnorm_bwd", "mde_pointwise_bwd_bn",
      "mde_batchnorm_bwd_apply", "mde_conv3x3_wgrad")),
    ("test_gpu_conv3x3", "test_fused_bn_relu_pointwise_branch_vs_float64",
     _k("cin,e,eo,h,w,train", [(3, 32, 16, 16, 48, False)]),
     ("mde_conv3x3_fwd", "mde_batchnorm_fwd_coef", "mde_pointwise_fwd", "mde_batchnorm_fwd_eval",
      "mde_batchnorm_bwd", "mde_pointwise_bwd_bn", "mde_batchnorm_bwd_apply", "mde_conv3x3_wgrad")),
    ("test_gpu_conv3x3", "test_fused_bn_relu_pointwise_branch_vs_float64",   # cin 64: no fused sums
     _k("cin,e,eo,h,w,train", [(64, 64, 64, 8, 64, True), (64, 64, 64, 8, 64, False)]),
     ("mde_batchnorm_fwd_coef", "mde_pointwise_bwd", "mde_batchnorm_bwd", "mde_conv3x3_wgrad")),
    ("test_gpu_conv3x3", "test_pointwise_bwd_bn_sums_match_separate_reduce",
     _k("cin,cout,n,h,w", [(32, 16, 3, 8, 64)]),
     ("mde_pointwise_bwd", "mde_batchnorm_bwd", "mde_pointwise_bwd_bn")),
    ("test_gpu_conv3x3", "test_bn_statistics_from_pointwise_epilogue",
     _k("cin,cout,n,h,w", [(32, 16, 3, 8, 64)]),
     ("mde_pointwise_fwd_stats", "mde_batchnorm_fwd_train_stats", "mde_batchnorm_fwd_train",
      "mde_batchnorm_fwd_coef")),
    ("test_gpu_conv3x3", "test_bn_statistics_from_conv_epilogue",
     _k("cin,cout,n,h,w,off", [(3, 32, 3, 37, 70, 0.0)]),
     ("mde_conv3x3_fwd_stats", "mde_batchnorm_fwd_train_stats", "mde_batchnorm_fwd_train")),
    # pointwise: one kernel instance per (cin, cout) of the shape list, fp32 and
    # bf16; h w % 64 == 0 is the only plane rule (no further variant by plane)
    ("test_gpu_parity", "test_pointwise_conv_vs_aten", _k("n,cin,cout,h,w", [
        (3,) + p + (8, 8) for p in _PW]), ("mde_pointwise_fwd", "mde_pointwise_bwd"), _PW_OK),
    # --------------------------------------------------- pointwise, deferred
    ("test_gpu_pw_deferred", "test_bn_form_fused_vs_separate", _k("cin,cout,n,h,w", [
        (ci, co) + s for ci, co in [(16, 16), (16, 8), (32, 32), (32, 16), (16, 32)]
        for s in [(2, 8, 8), (3, 8, 24)]]),
     ("mde_batchnorm_bwd_apply", "mde_pointwise_bwd_bn", "mde_batchnorm_bwd_coef",
      "mde_pointwise_bwd_bn_deferred")),
    ("test_gpu_pw_deferred", "test_se_form_fused_vs_separate", _k("cin,cout,n,h,w", [
        (ci, co) + s for ci, co in [(16, 16), (16, 8), (32, 32), (32, 16), (16, 32)]
        for s in [(2, 8, 8), (3, 8, 24)]]),
     ("mde_se_bn_fwd", "mde_se_bn_bwd", "mde_pointwise_bwd_bn", "mde_se_bn_bwd_coef",
      "mde_pointwise_bwd_bn_deferred")),
    ("test_gpu_pw_deferred", "test_bn_form_bit_identical_at_plane_size", _k("cin,cout", [
        (16, 16), (16, 8), (32, 32), (32, 16)]),
     ("mde_batchnorm_bwd_apply", "mde_batchnorm_bwd_coef", "mde_pointwise_bwd_bn_deferred")),
    ("test_gpu_pw_deferred", "test_se_form_bit_identical_at_plane_size", _k("cin,cout", [
        (16, 16), (16, 8), (32, 32), (32, 16)]),
     ("mde_se_bn_bwd", "mde_se_bn_bwd_coef", "mde_pointwise_bwd_bn_deferred")),
    ("test_gpu_abi_guard", "check_block_deferred_relocated", [{}],
     ("mde_batchnorm_bwd_coef", "mde_se_bn_bwd_coef", "mde_pointwise_bwd_bn_deferred",
      "mde_skip_reduce_bn_fwd", "mde_skip_reduce_bn_bwd")),
    # ------------------------------------------------- conv3x3 fp32 and bf16
    ("test_gpu_conv3x3", "test_conv3x3_vs_float64_oracle", _k("cin,cout,n,h,w", [
        p + (2, 9, 37) for p in [(16, 16), (32, 32)]]), _C3),
    ("test_gpu_conv3x3", "test_conv3x3_vs_float64_oracle", _k("cin,cout,n,h,w", [   # image input: no gx
        p + (2, 9, 37) for p in [(3, 16), (3, 32), (3, 64)]]), ("mde_conv3x3_fwd", "mde_conv3x3_wgrad")),
    ("test_gpu_conv3x3", "test_conv3x3_bf16_vs_float64_oracle", _k("cin,cout,n,h,w", [
        (16, 16, 1, 13, 72), (32, 32, 1, 13, 72), (16, 16, 1, 1, 4), (32, 32, 1, 1, 4)]), _C3),
    ("test_gpu_conv3x3", "test_conv3x3_bf16_stats_epilogue", _k("cin,cout", [(16, 16), (32, 32)]),
     ("mde_conv3x3_fwd_stats",)),
    ("test_gpu_conv3x3", "test_conv3x3_wgrad_c32_strips_vs_float64", _k("n,h,w", [(1, 7, 80)]),
     ("mde_conv3x3_wgrad",)),
    ("test_gpu_conv3x3", "test_conv3x3_wide_wgrad_vs_float64_oracle",
     # the generic kernel (two shapes), then the fixed strips of 80 / 40 / 20 columns
     _k("cin,cout,n,h,w", [(64, 64, 3, 1, 5), (32, 128, 1, 9, 21), (64, 64, 1, 9, 160),
                           (32, 64, 2, 5, 40), (32, 64, 3, 7, 20)]), ("mde_conv3x3_wgrad",), _C3W_OK),
    ("test_gpu_conv3x3", "test_conv3x3_wide_wgrad_padded_channels_vs_float64",   # strips 20 / 80 / 40
     _k("cin,cout,n,h,w", [(56, 64, 2, 9, 20), (40, 256, 2, 17, 80), (24, 64, 3, 5, 40)]),
     ("mde_conv3x3_wgrad",), _C3W_OK),
    # -------------------------------------------------------------------- wino
    # wino_launch picks by cout (16- / 32- / 64-channel blocks: 16 -> 16 has its own
    # 8 x 32-pixel column blocking), by padded channels, by the persistent plane
    # test and by the XCD split of weight-heavy shapes (64 -> 256 at 15 x 20: split 4)
    ("test_gpu_wino", "test_wino_abi_vs_float64_oracle", _k("cin,cout,h,w", [
        (16, 32, 10, 18), (16, 16, 40, 70), (64, 256, 15, 20)]),
     ("mde_wino_weight", "mde_wino_conv"), _WINO_OK),
    ("test_gpu_wino", "test_wino_stats_epilogue", _k("cin,cout,h,w", [
        (32, 32, 9, 36), (16, 16, 40, 64), (64, 256, 15, 20)]),
     ("mde_wino_conv_stats",), _WINO_OK),
    ("test_gpu_wino", "test_wino_weight2_matches_both_transforms", [{}],
     ("mde_wino_weight2", "mde_wino_weight")),
    ("test_gpu_wino", "test_wino_weight_table_matches_weight2", [{}],
     ("mde_wino_weight_table", "mde_wino_weight2")),
    ("test_gpu_wino", "test_wino_conv_acc_is_conv_plus_add", _k("cin,cout,h,w", [(64, 64, 9, 40)]),
     ("mde_wino_conv_acc",)),
    ("test_gpu_wino", "test_wino_padded_channels_vs_float64",
     _k("cin,cout,h,w", [(24, 32, 9, 18), (40, 64, 11, 30)]), ("mde_wino_weight", "mde_wino_conv_stats")),
    ("test_gpu_wino", "test_wino_persistent_bitwise", _k("cin,cout,h,w,n", [
        (16, 32, 10, 18, 3), (32, 96, 7, 34, 2), (64, 64, 9, 40, 3), (16, 16, 40, 70, 2),
        (64, 256, 15, 20, 3)]), ("mde_wino_conv",), _WINO_OK),
    ("test_gpu_wino", "test_wino_position_split_vs_float64", _k("cin,cout,h,w,n", [
        (16, 32, 10, 18, 3), (32, 96, 7, 34, 2)]), ("mde_wino_conv",)),
    # ------------------------------------------- stride 2 / wide stride 1
    ("test_gpu_conv3x3s2", "test_conv3x3s2_hip_kernels_below_the_dispatch_threshold",
     _k("cin,cout,h,w", [(64, 64, 7, 10)]), ("mde_conv3x3s2_fwd", "mde_conv3x3s2_bwd_data")),
    ("test_gpu_conv3x3s2", "test_conv3x3s2_stem_3_channels", _k("h,w", [(66, 256)]),
     ("mde_conv3x3s2_fwd", "mde_conv3x3s2_wgrad")),
    ("test_gpu_conv3x3", "test_conv3x3s2_wgrad_vs_float64", _k("cin,cout,n,h,w", [   # last: 32 -> 32 strips
        (32, 32, 2, 2, 64), (3, 32, 1, 9, 130), (32, 32, 1, 5, 80)]), ("mde_conv3x3s2_wgrad",), _S2W_OK),
    ("test_gpu_conv3x3", "test_conv3x3s2_wide_wgrad_vs_float64",     # strips of 40, then of 20
     _k("cin,cout,n,h,w", [(64, 128, 1, 37, 80), (32, 64, 2, 9, 40)]), ("mde_conv3x3s2_wgrad",), _S2W_OK),
    ("test_gpu_conv3x3s2", "test_conv3x3_wide_s1_vs_float64_oracle", _k("cin,cout,h,w", [
        (128, 128, 8, 10), (64, 64, 9, 40)]), ("mde_conv3x3_wide_fwd", "mde_conv3x3_wide_bwd_data")),
    # ----------------------------------------------------------------- conv1x1
    ("test_gpu_conv1x1", "test_conv1x1_vs_float64_oracle", _k("cin,cout,stride,h,w", [
        (96, 160, 1, 6, 6), (40, 120, 1, 6, 8), (64, 96, 2, 15, 20), (40, 24, 2, 13, 24),
        # One row set for every kernel instance the 1x1 dispatchers can pick
        # (C1_INSTANCES below: the channel mix's M tiles, padded or not, both
        # passes and strides; the small mix's MT 1..8 of both passes; the weight
        # gradient's six block tiles at both strides and its ten small-channel wave
        # tiles).  Which row selects which is not written here: c1_variants mirrors
        # the dispatch rules and test_abi_guard_host.py asserts that the rows reach
        # exactly C1_INSTANCES.
        (512, 128, 1, 8, 10), (256, 64, 1, 15, 20), (128, 64, 1, 6, 8), (64, 128, 1, 6, 8),
        (64, 64, 1, 6, 8), (240, 80, 1, 6, 8), (128, 256, 2, 30, 40),
        (16, 16, 1, 6, 8), (24, 16, 1, 6, 8), (56, 16, 1, 6, 8), (120, 16, 1, 6, 8),
        (16, 24, 1, 6, 8), (24, 24, 1, 6, 8), (56, 24, 1, 6, 8), (16, 56, 1, 6, 8),
        (24, 56, 1, 6, 8), (16, 120, 1, 6, 8),
        (72, 40, 1, 6, 8), (64, 104, 1, 6, 8), (32, 64, 2, 12, 16), (40, 72, 1, 6, 8),
        (24, 192, 1, 6, 8), (16, 64, 2, 12, 16), (64, 16, 2, 12, 16), (16, 88, 1, 6, 8),
        (88, 16, 1, 6, 8), (104, 16, 1, 6, 8), (16, 128, 2, 12, 16), (128, 16, 2, 12, 16),
        (16, 256, 1, 6, 8), (64, 64, 2, 12, 16), (256, 16, 1, 6, 8), (64, 128, 2, 12, 16),
        (128, 64, 2, 12, 16), (24, 104, 1, 6, 8), (64, 96, 1, 6, 8)]),
     ("mde_conv1x1_fwd", "mde_conv1x1_bwd_data", "mde_conv1x1_wgrad"), _C1_OK),
    ("test_gpu_conv1x1", "test_conv1x1_stride2_zero_fills_odd_positions", [{}],
     ("mde_conv1x1_bwd_data",)),
    ("test_gpu_conv1x1", "test_conv1x1_mix_small_writes_every_output", _k("cin,cout,h,w", [
        (16, 16, 10, 14), (24, 72, 7, 12), (40, 120, 9, 20), (64, 24, 4, 9), (120, 40, 5, 16)]),
     ("mde_conv1x1_fwd",)),
    # -------------------------------------------------------------- bf16 convs
    # convbf picks its tiles from the plane and the LDS room (resident filter with
    # 64 x 64 or 32 x 64 wave tiles, else the chunked kernel with 2 or 1 M tiles a
    # wave, 32- or 64-channel blocks); the file's SHAPES name one plane per tile
    # choice, so all of them under the size limit run here (the check body asserts
    # convbf_ok, i.e. mde_convbf_supported for the three passes, itself)
    ("test_gpu_convbf", "test_convbf_vs_float64_oracle", _k("cin,cout,h,w,k,s", [
        (64, 32, 18, 24, 3, 1), (128, 128, 8, 10, 3, 1), (96, 64, 22, 40, 3, 2),
        (512, 128, 8, 10, 1, 1), (256, 512, 15, 20, 1, 2),
        (64, 64, 60, 80, 3, 1), (128, 128, 30, 40, 3, 1), (256, 256, 15, 20, 3, 1),
        (128, 64, 60, 80, 3, 1), (32, 64, 120, 160, 3, 2), (64, 128, 60, 80, 3, 2),
        (128, 256, 30, 40, 3, 2), (256, 256, 15, 20, 3, 2), (64, 64, 60, 80, 1, 1),
        (64, 128, 60, 80, 1, 1), (640, 256, 8, 10, 1, 1), (32, 64, 120, 160, 1, 2),
        (96, 64, 26, 160, 3, 2)]),
     ("mde_convbf_pack_both", "mde_convbf_fwd", "mde_convbf_bwd_data", "mde_convbf_wgrad")),
    ("test_gpu_convbf", "test_convbf_pack_single_matches_layout_and_pack_both",
     _k("cin,cout,k", [(32, 32, 1), (96, 64, 3)]), ("mde_convbf_pack", "mde_convbf_pack_both")),
    ("test_gpu_convbf", "test_convbf_epilogue_statistics", _k("cin,cout,h,w,k,s", [
        (64, 32, 18, 24, 3, 1), (128, 128, 8, 10, 3, 1), (96, 64, 22, 40, 3, 2),
        (512, 128, 8, 10, 1, 1), (256, 512, 15, 20, 1, 2)]),
     ("mde_convbf_fwd",)),
    ("test_gpu_convbf", "test_convbf_pack_scope_matches_per_conv_pack", [{}],
     ("mde_convbf_pack_table",)),
    ("test_gpu_stem", "test_stem_vs_float64_oracle", _k("n,cout,h,w", [(3, 32, 37, 52)]),
     ("mde_stem_bf16_fwd", "mde_stem_bf16_wgrad")),
    ("test_gpu_stem", "test_guide_conv_weight_gradient_from_bf16_gy",
     _k("n,cout,h,w", [(2, 32, 30, 44)]), ("mde_conv3x3_guide_bf16_wgrad",)),
    ("test_gpu_bf16", "test_guide_conv_bf16_matches_rounded_fp32_kernel",
     _k("cout,h,w", [(16, 21, 36)]), ("mde_conv3x3_guide_bf16_fwd",)),
    ("test_gpu_bf16", "test_bnrelu_pointwise_bf16_storage_matches_fp32_kernel",
     _k("cin,cout,n,h,w", [(64, 32, 2, 30, 64), (32, 64, 2, 30, 64), (64, 64, 2, 30, 64)]),
     ("mde_batchnorm_fwd_coef", "mde_pointwise_fwd"), _PW_OK),
    ("test_gpu_bf16", "test_pointwise_bf16_products_vs_float64",
     # (its plane is fixed: the 64-channel shapes are over the size limit here and
     # run in the storage check above instead)
     _k("cin,cout,bnr", [p + (True,) for p in _PW if max(p) < 64]),
     ("mde_pointwise_fwd", "mde_pointwise_bwd_bn")),
    ("test_gpu_bf16", "test_pointwise_bf16_products_vs_float64",
     _k("cin,cout,bnr", [p + (False,) for p in _PW if max(p) < 64]),
     ("mde_pointwise_fwd", "mde_pointwise_bwd")),
    ("test_gpu_bf16", "test_skip_reduce_bf16_storage_matches_fp32_kernel",
     _k("cin,cout,n,h,w", [(32, 16, 3, 48, 64)]), ("mde_skip_reduce_fwd", "mde_skip_reduce_bwd")),
    ("test_gpu_bf16", "test_skip_reduce_bn_bf16_storage_matches_fp32_kernel",
     _k("cin,cout,n,h,w", [(4, 1, 2, 30, 40)]), ("mde_skip_reduce_bn_fwd", "mde_skip_reduce_bn_bwd")),
    ("test_gpu_bf16", "test_se_bn_cat_bf16_storage_matches_fp32_kernel",
     _k("ca,cb,n,h,w", [(32, 32, 2, 30, 40)]), ("mde_se_bn_fwd", "mde_se_bn_bwd")),
    ("test_gpu_bf16", "test_bilinear_x2_bf16_storage_matches_fp32_kernel",
     _k("c,h,w", [(8, 15, 21)]), _BF),
    ("test_gpu_bf16", "test_bilinear_generic_bf16_storage_matches_fp32_kernel",
     _k("c,hi,wi,ho,wo,align", [(32, 4, 5, 8, 10, False)]), _BF),
    # ------------------------------------------------------------ head / dwconv
    ("test_gpu_head", "test_head_conv_vs_float64", _k("n,c,h,w", [(2, 40, 7, 12), (3, 3, 1, 4)]),
     ("mde_head_conv_fwd", "mde_head_conv_dgrad", "mde_head_conv_wgrad")),
    ("test_gpu_dwconv", "test_dwconv_matches_aten", _k("n,c,h,w,k,s", [
        (1, 8, 7, 9, 3, 2), (1, 3, 33, 67, 5, 2), (2, 5, 17, 130, 3, 1), (9, 2, 4, 6, 3, 1)]),
     ("mde_dwconv_fwd", "mde_dwconv_bwd")),
    ("test_gpu_dwconv", "test_dwconv_other_padding", _k("n,c,h,w,k,s,p", [
        (2, 8, 30, 41, 5, 2, 1), (1, 6, 19, 70, 5, 1, 4)]), ("mde_dwconv_fwd", "mde_dwconv_bwd")),
    ("test_gpu_dwconv", "test_dwconv_single_gradient", _k("which", ["gx", "gw"]),
     ("mde_dwconv_fwd", "mde_dwconv_bwd")),
    # streaming in whole rows (no edge loads); 2 V0 columns a lane at stride 2 with an odd
    # height (rows past H / HO); one-lane EDGE segments; a channel split over blocks (the check
    # also requests gw alone: dw_wsum_kernel); a short last stack of planes in the strip kernels
    ("test_gpu_dwconv", "test_dwconv_instance", _k("n,c,h,w,k,s,p", [
        (2, 3, 9, 16, 3, 1, 1), (2, 3, 9, 168, 3, 2, 1), (2, 3, 5, 92, 5, 1, 2),
        (3, 2, 40, 320, 3, 1, 1), (30, 1, 7, 9, 3, 2, 1)]), ("mde_dwconv_fwd", "mde_dwconv_bwd")),
    # ---------------------------------------------------------------- batchnorm
    ("test_gpu_bn", "test_batchnorm_train_matches_aten", _k("shape,act,res", [
        (s,) + ar for s in [(2, 8, 3, 5), (3, 7, 1, 1), (32, 64, 2, 3), (200, 8, 3, 7), (16, 8, 16, 60),
                            (4, 16, 30, 40)] for ar in [("relu", True), ("hardswish", False)]]),
     ("mde_batchnorm_fwd_train", "mde_batchnorm_bwd")),
    ("test_gpu_bn", "test_batchnorm_eval_matches_aten", _k("act,res", [
        ("relu", False), ("none", True), ("hardswish", False)]),
     ("mde_batchnorm_fwd_eval", "mde_batchnorm_bwd")),
    ("test_gpu_bn", "test_conv_bias_folded_into_bn", _k("train", [True, False]),
     ("mde_batchnorm_bwd",)),
    ("test_gpu_bn", "test_batchnorm_bf16_storage_matches_fp32_kernel",
     _k("shape,act,res", [((2, 8, 3, 5), "relu", True)]),
     ("mde_batchnorm_fwd_train", "mde_batchnorm_bwd")),
    ("test_gpu_bn", "test_batchnorm_bf16_one_launch_matches_two_launch", _k("shape,act,res", [
        ((2, 512, 1, 1), "relu", True), ((2, 128, 2, 3), "none", False)]),
     ("mde_batchnorm_fwd_train", "mde_batchnorm_bwd")),
    # --------------------------------------------------------------- NewCRF / SAM
    ("test_gpu_newcrf", "test_layernorm_matches_aten", _k("rows,c", [
        (37, 512), (1, 128), (50, 192), (98, 64)]), ("mde_layernorm_fwd", "mde_layernorm_bwd")),
    ("test_gpu_newcrf", "test_add_layernorm_bitwise_vs_separate_add", _k("rows,c", [(50, 192)]),
     ("mde_layernorm_add_fwd", "mde_layernorm_bwd_res")),
    ("test_gpu_newcrf", "test_token_transposes_bit_exact", _k("shape", [(1, 5, 7, 3), (2, 40, 7, 12)]),
     ("mde_transpose",)),
    ("test_gpu_newcrf", "test_colsum_and_gelu_bwd_colsum_vs_float64", _k("t,n", [(257, 12)]),
     ("mde_colsum", "mde_gelu_bwd_colsum")),
    ("test_gpu_newcrf", "test_window_attention_vs_oracle", _k("b,h,w,emb,heads", [
        (3, 9, 16, 64, 2), (2, 7, 7, 128, 4)]), ("mde_window_attn_fwd", "mde_window_attn_bwd")),
    ("test_gpu_newcrf", "test_newcrf_golden", _k("case", [NEWCRF_CASES[4]]),
     ("mde_window_attn_fwd", "mde_window_attn_bwd", "mde_layernorm_add_fwd", "mde_layernorm_bwd_res",
      "mde_transpose")),
    ("test_gpu_linear", "test_linear_wgrad_vs_float64", _k("t,m,n,bias", [
        (16, 128, 128, True), (16, 128, 128, False)]), ("mde_linear_wgrad",)),
    ("test_gpu_linear", "test_chansum_vs_float64", _k("n,c,h,w", [(1, 40, 2, 2), (5, 7, 6, 10)]),
     ("mde_chansum",)),
    ("test_gpu_sam", "test_sam_block_vs_oracle", _k("b,h,w,emb,heads", [(2, 7, 7, 128, 4)]),
     ("mde_window_attn_fwd", "mde_window_attn_bwd")),
    ("test_gpu_sam", "test_sam_golden", _k("case", [SAM_CASES[3]]),
     ("mde_window_attn_fwd", "mde_window_attn_bwd")),
    # the generic-window instances (window != 7): 8 fills the 64-token tile, 4 leaves slots beyond it
    ("test_gpu_attn_paths", "test_generic_window", _k("b,h,w,heads,ws,shift", [
        (2, 9, 11, 3, 8, 4), (2, 9, 11, 3, 4, 2)]), ("mde_window_attn_fwd", "mde_window_attn_bwd")),
    ("test_gpu_attn_paths", "test_generic_window_v_bias", _k("b,h,w,heads,ws,shift", [
        (2, 9, 11, 3, 8, 0)]), ("mde_window_attn_fwd", "mde_window_attn_bwd")),
    # --------------------------------------------------- losses, metrics, data
    ("test_gpu_parity", "test_ssim_golden", _k("tag", ["rand", "close", "anti"]), ("mde_ssim3_l1_fwd",)),
    ("test_gpu_parity", "test_ssim_l1_vs_oracle_sizes", _k("shape", [
        (1, 1, 2, 2), (1, 2, 5, 7), (3, 1, 17, 70), (2, 1, 50, 260), (2, 1, 36, 132), (1, 1, 3, 3),
        (1, 1, 2, 121), (2, 1, 130, 61), (1, 1, 97, 2), (4, 1, 64, 120)]),
     ("mde_ssim3_l1_fwd", "mde_minmax")),
    ("test_gpu_parity", "test_train_objective_golden", [{}],
     ("mde_ssim3_l1_fwd", "mde_minmax", "mde_depthnorm_apply")),
    ("test_gpu_parity", "test_depth_loss_golden",
     _k("tag", ["dl_alh", "dl_mask", "dl_small", "dl_ssim_only"]),
     ("mde_depth_loss_fwd", "mde_depth_loss_bwd")),
    ("test_gpu_parity", "test_depth_loss_streaming_shapes_vs_oracle", _k("shape,params", [
        ((2, 1, 100, 130), (0.1, 1.0, 1.0, 10.0)), ((1, 2, 11, 11), (0.1, 1.0, 1.0, 10.0)),
        ((3, 1, 45, 55), (0.0, 1.0, 0.0, 1.0)), ((2, 1, 70, 108), (0.5, 0.0, 1.0, 10.0)),
        ((2, 1, 64, 97), (1.0, 0.0, 0.0, 10.0))]), ("mde_depth_loss_fwd", "mde_depth_loss_bwd")),
    ("test_gpu_metrics", "test_batch_errors_match_reference", [{}], ("mde_eval_sums",)),
    ("test_gpu_metrics", "test_compute_errors_matches_reference", [{}], ("mde_eval_sums",)),
    ("test_gpu_metrics", "test_empty_selection_is_nan", [{}], ("mde_eval_sums",)),
    ("test_gpu_data", "test_batch_kernel_matches_reference", [{}], ("mde_nyu_augment",)),
]

# ------------------------------------------------------------------------------
# Variant census: plain-Python mirrors of the shape rules by which two
# dispatchers pick a kernel instance (csrc/conv1x1.hip: mix_small_mt, cm_bm,
# small_plan, wg_plan; csrc/conv3x3.hip: wide_fixed_sw, wide_s2_sw, c32_s2).
# test_abi_guard_host.py asserts with them that the rows above reach every
# instance; if a rule changes in the kernels, change it here and re-derive the rows.
def _cdiv(a, b):
    return -(-a // b)


def _c1_mix_mt(m, k):
    if m > 128 or k > 128 or (m % 32 == 0 and k % 32 == 0):
        return 0
    mt = _cdiv(m, 16)
    return mt if k * (16 * mt + (16 if mt % 2 == 0 else 0)) <= 8192 else 0


def _c1_small_tile(ci, co, q):
    co16, ci16 = _cdiv(co, 16), _cdiv(ci, 16)
    if q % 16 or (ci % 32 == 0 and co % 32 == 0) or co16 * ci16 > 24:
        return None
    best, tile = 1 << 30, None
    for mt in (1, 2, 4, 8):
        for nt in (1, 2, 4, 8):
            groups = _cdiv(co16, mt) * _cdiv(ci16, nt)
            if mt * nt <= 8 and groups <= 3 and groups * mt * nt < best:   # first of equal waste
                best, tile = groups * mt * nt, (mt, nt)
    return tile


def _c1_bm(m):
    return 128 if m % 128 == 0 else (64 if m % 64 == 0 else 32)


def c1_variants(cin, cout, stride, h, w):
    """The kernel instances the three conv1x1 passes take at this shape."""
    q = ((h - 1) // stride + 1) * ((w - 1) // stride + 1)
    out = set()
    for what, m, k in (("fwd", cout, cin), ("dgrad", cin, cout)):
        if stride == 1 and _c1_mix_mt(m, k):
            out.add(("mix_small", what, _c1_mix_mt(m, k)))
        else:
            out.add(("mix", what, stride, _c1_bm(m), bool(k % 32 or m % _c1_bm(m))))
    small = _c1_small_tile(cin, cout, q) if stride == 1 else None
    if small:
        out.add(("wgrad_small",) + small)
    else:
        a, b = _c1_bm(cout), _c1_bm(cin)
        out.add(("wgrad", stride) + ((128, 32) if b == 32 else (32, 128) if a == 32 else (a, b)))
    return out


C1_INSTANCES = (
    {("mix_small", p, mt) for p in ("fwd", "dgrad") for mt in range(1, 9)}
    | {("mix", p, s, bm, pad) for p in ("fwd", "dgrad") for s in (1, 2) for bm in (128, 64, 32)
       for pad in (False, True)}
    | {("wgrad_small", mt, nt) for mt in (1, 2, 4, 8) for nt in (1, 2, 4, 8) if mt * nt <= 8}
    | {("wgrad", s) + t for s in (1, 2)
       for t in ((128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (32, 128))})


def c3_wide_variant(cin, cout, stride, w):
    """The wide 3x3 weight gradient's kernel at this input width: (strip columns or
    0 for the generic kernel, input channels padded)."""
    if stride == 1:
        sw = 80 if w % 80 == 0 else (w if w in (40, 20) else 0)
    else:
        wo = (w - 1) // 2 + 1
        if cin == 32 and cout == 32:
            return ("c32", 40) if wo % 40 == 0 else ("c32", 0)
        sw = 40 if wo % 40 == 0 else (20 if wo == 20 else 0)
    return (sw, cin % 32 != 0)


MAX_ELEMENTS = 2 << 20   # no tensor of a guarded case is larger


def check_block_deferred_relocated(monkeypatch, guard):
    """The Guided_Upsampling_Block backward of test_gpu_pw_deferred's block test
    (out_features = 1, the deferred route) under guard: the test's own float64
    comparison, against its apply-pass run made unguarded, and bitwise equal to
    an unguarded deferred run.  (That test also counts launches, which a harness
    that runs every launch twice doubles, so its body cannot run here as it is.)"""
    from tests.test_gpu_pw_deferred import _block_case, _block_compare, _block_reference
    monkeypatch.setenv("MDE_PW_DEFER", "1")
    got, _ = _block_case(1, 2, 8, 16)
    with guard.paused():
        same, _ = _block_case(1, 2, 8, 16)
        monkeypatch.setenv("MDE_PW_DEFER", "0")
        apply_pass, _ = _block_case(1, 2, 8, 16)
    _block_compare(apply_pass, got, _block_reference(1, 2, 8, 16))
    for k in sorted(same):
        assert torch.equal(got[k], same[k]), k


def _cases():
    out = []
    for mod, fn, rows, entries, *q in FAMILIES:
        for kw in rows:
            tag = "-".join(str(v[0] if isinstance(v, tuple) and v and isinstance(v[0], str) else v)
                           for v in kw.values()).replace(" ", "")
            out.append(pytest.param(mod, fn, kw, entries, q[0] if q else None, id=f"{fn.split('_', 1)[1]}[{tag}]"))
    return out


def declared_entries():
    """The entries the guarded cases declare (the static coverage test's input)."""
    return {e for fam in FAMILIES for e in fam[3]}


@pytest.mark.parametrize("mod,fn,kw,entries,supported", _cases())
def test_guarded(mod, fn, kw, entries, supported, golden, monkeypatch):
    check = getattr(importlib.import_module(f"tests.{mod}"), fn)
    if supported is not None:
        from monocular_depth_estimation_amd import _abi
        query, args = supported(kw)
        assert _abi.query(query, *args) > 0, (query, args)
    kw = dict(kw)
    params = inspect.signature(check).parameters
    if "golden" in params:
        kw["golden"] = golden
    if "monkeypatch" in params:
        kw["monkeypatch"] = monkeypatch
    with guarded_abi() as g:
        if "guard" in params:
            kw["guard"] = g
        check(**kw)
    assert g.max_numel <= MAX_ELEMENTS, g.max_numel
    missing = set(entries) - set(g.calls)
    assert not missing, f"{fn} {kw}: never called {sorted(missing)} (called: {dict(g.calls)})"
