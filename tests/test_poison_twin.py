"""The poison tier on the CPU twin: the self-tests of tests/poison.py, and the kernel-family bodies of the twin tier
(tests/test_cpu_twin.py, at its shapes) re-run with every `torch.empty` / `torch.empty_like` result and every `lib.workspace` buffer
poisoned and fenced.  What the bodies assert is unchanged; afterwards the canary bands must be intact.  A failure here means a Python
shell, the twin or a reference depends on what was in the memory it was given; on the GPU (tests/test_gpu_unwritten.py) the same run
then isolates the HIP kernels and their workspace contracts."""
import pytest
import torch

import conv_patterns as GRIDS
import gemm_forms as GEMM
import poison
from poison import poisoned, run_poisoned
from test_cpu_twin import on_cpu  # noqa: F401  (fixture)
import test_gpu_losses as LOSS
import test_gpu_modules as M
import test_gpu_ops as OPS
import test_evaluation as EV
import test_mesh_reference as MESH
import test_render_stages as RS
import geometry_reference as GR

golden_latents = RS.golden_latents
net = RS.net


# ---- the helper itself (pure Python: no kernel is made to misbehave) ---------------------------------------------------------------
def _fake_op(x, skip=None):
    """An "op" that writes its torch.empty result element by element and may forget one."""
    y = torch.empty_like(x)
    flat = y.view(-1)
    for i in range(x.numel()):
        if i != skip:
            flat[i] = 2.0 * float(x.view(-1)[i])
    return y


def test_unwritten_element_is_caught_by_the_nan_check():
    x = torch.arange(12.0).reshape(3, 4)
    with poisoned():
        full, holed = _fake_op(x), _fake_op(x, skip=7)
    assert not torch.isnan(full).any() and torch.equal(full, 2 * x)
    assert torch.isnan(holed).view(-1).nonzero().flatten().tolist() == [7]
    with poisoned():
        ints = torch.empty(5, dtype=torch.int64)
        like = torch.empty_like(ints, dtype=torch.int32)
        flags = torch.empty(3, dtype=torch.bool)
    assert ints.tolist() == [-1] * 5 and like.tolist() == [-1] * 5 and flags.tolist() == [True] * 3
    assert poison.fill_byte(torch.int32, torch.device("cuda", 0)) == 0 and poison.fill_byte(torch.float32, torch.device("cuda", 0)) == 0xFF


def test_a_store_into_the_band_is_caught():
    with poisoned() as p:
        t = torch.empty((4, 5), dtype=torch.float32)
        ws = poison._workspace("splitk", 1000, torch.device("cpu"))
        p.check_canaries()
        base = p.records[0][0]
        assert base.numel() == 2 * poison.BAND + 80 and t.data_ptr() == base.data_ptr() + poison.BAND
        base[poison.BAND + 80] = 0           # one byte past the end of t
        with pytest.raises(poison.CanaryError, match=r"torch.empty\(\(4, 5\), float32\).*0 byte\(s\) before it, 1 after"):
            p.check_canaries()
        base[poison.BAND + 80] = poison.CANARY
        base[poison.BAND - 1] = 0            # one byte in front of it
        with pytest.raises(poison.CanaryError, match="1 byte"):
            p.check_canaries()
        base[poison.BAND - 1] = poison.CANARY
        p.check_canaries()
        wbase = p.records[1][0]
        assert ws.numel() == 1000 and wbase.numel() == 1000 + poison.BAND and bool((ws == 0xFF).all())
        wbase[1000] = 1
        with pytest.raises(poison.CanaryError, match="workspace"):
            p.check_canaries()
        wbase[1000] = poison.CANARY
        p.renew()                            # the blocks are scribbled over and released
        assert p.records == [] and float(t[0, 0]) > 1e38 and int(ws[0]) == poison.SCRIBBLE


def test_wrapper_is_transparent():
    import shapegan_amd.lib as L
    import shapegan_amd.ops as ops
    real = (torch.empty, torch.empty_like, L.workspace, ops.workspace)
    src = torch.zeros(3, 5, 7, dtype=torch.float64)
    with poisoned() as p:
        assert L.workspace is ops.workspace and L.workspace is not real[2]
        cases = [(torch.empty(3, 5), (3, 5), torch.float32), (torch.empty((2, 3, 4), dtype=torch.int32), (2, 3, 4), torch.int32),
                 (torch.empty(size=(7,), dtype=torch.float64, device="cpu"), (7,), torch.float64),
                 (torch.empty(torch.Size((1, 1)), dtype=torch.uint8), (1, 1), torch.uint8),
                 (torch.empty(0), (0,), torch.float32), (torch.empty((), dtype=torch.long), (), torch.int64),
                 (torch.empty_like(src), (3, 5, 7), torch.float64), (torch.empty_like(src, dtype=torch.float32), (3, 5, 7), torch.float32),
                 (torch.empty(5, requires_grad=True), (5,), torch.float32)]
        for t, shape, dtype in cases:
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous()
            assert t.data_ptr() % 16 == 0
        assert cases[-1][0].requires_grad and cases[-1][0].is_leaf
        # forms the guard does not model: a plain poisoned allocation with the real allocator's layout
        cl = torch.empty((2, 3, 4, 4), memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last) and torch.isnan(cl).all()
        tr = torch.empty_like(src.transpose(0, 2))
        assert tr.stride() == src.transpose(0, 2).stride() and torch.isnan(tr).all()
        out = torch.zeros(4)
        assert torch.empty(4, out=out) is out and torch.isnan(out).all()
        ws = L.workspace("bn", 10, torch.device("cpu"))
        assert ws.dtype == torch.uint8 and ws.numel() == 256 and ws.data_ptr() % 16 == 0 and ws.is_contiguous()
        assert L.workspace("bn", 10, torch.device("cpu")).data_ptr() != ws.data_ptr()      # fresh every time while ws is alive
        assert L.tickets("poison-self-test", torch.device("cpu")).tolist() == [0] * 16            # state: left alone
        p.check_canaries()
    assert (torch.empty, torch.empty_like, L.workspace, ops.workspace) == real
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned():
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, L.workspace, ops.workspace) == real and poison.active() is None


# ---- the bodies of the twin tier under poison --------------------------------------------------------------------------------------
BODIES = [
    (OPS.test_conv3d_fwd_dgrad_wgrad, (2, 3, 5, 8)), (OPS.test_conv3d_fwd_dgrad_wgrad, (1, 1, 4, 6)),
    (OPS.test_conv3d_fwd_dgrad_wgrad, (3, 8, 1, 4)), (OPS.test_conv3d_fwd_dgrad_wgrad, (1, 2, 2, 2)),
    (OPS.test_conv3d_fwd_dgrad_wgrad, (2, 24, 48, 8)),
    (OPS.test_conv_transpose3d, (2, 16, 8, 4)), (OPS.test_conv_transpose3d, (3, 8, 1, 8)), (OPS.test_conv_transpose3d, (1, 5, 3, 3)),
    (OPS.test_conv_wgrad_through_activation, (2, 5, 4, 1)), (OPS.test_conv_wgrad_through_activation, (1, 3, 2, 2)),
    (OPS.test_conv_from_sdf_zero_channels, ()),
    (OPS.test_conv_transpose3d_to_one_channel_streaming_kernel_random_shapes, ()),
    *GRIDS.DISPATCH_BODIES,          # (the conv family on grids of three different extents: tests/test_gpu_conv_grids.py)
    (OPS.test_linear_fwd_bwd, (64, 128, 256)), (OPS.test_linear_fwd_bwd, (4, 128, 256)), (OPS.test_linear_fwd_bwd, (5, 7, 3)),
    (OPS.test_gemm_double_backward, ()),
    # (the GEMM family against float64: tests/test_gpu_gemm_forms.py)
    *[(GEMM.body_gemm, (i,)) for i in GEMM.POISON_TWIN_IDS], *[(GEMM.body_gemm_nt, (i,)) for i in GEMM.NT_POISON_IDS],
    (GEMM.body_rowsum, GEMM.ROWSUM_CASES[0]), (GEMM.body_rowsum_multi, GEMM.ROWSUM_MULTI_CASES[1]),
    (GEMM.body_segsum, GEMM.SEGSUM_CASES[1]), (GEMM.body_colsum, GEMM.COLSUM_CASES[3]),
    (OPS.test_batchnorm_train_fwd_bwd, (4, 8, 64)), (OPS.test_batchnorm_train_fwd_bwd, (4, 256, 1)),
    (OPS.test_batchnorm_train_fwd_bwd, (3, 7, 27)),
    (OPS.test_activations, ()), (OPS.test_mean_reduction, ()), (OPS.test_gather_scatter_rows_bit_exact, ()),
    (OPS.test_rmsprop_adam_clamp_match_torch, ()),
    (OPS.test_sdfnet_points_mode, (1, 128)), (OPS.test_sdfnet_points_mode, (63, 128)), (OPS.test_sdfnet_points_mode, (777, 256)),
    (OPS.test_sdfnet_points_mode, (130, 16)),
    (OPS.test_sdfnet_shapes_mode, (3, 512)), (OPS.test_sdfnet_shapes_mode, (1, 37)),
    (OPS.test_sdfnet_segments_mode, (5, 700)), (OPS.test_sdfnet_segments_mode, (3, 64)), (OPS.test_sdfnet_segments_mode, (7, 33100)),
    (OPS.test_sdf_batch_sort, (5, 40, 700)), (OPS.test_sdf_batch_sort, (300, 7, 1000)), (OPS.test_sdf_batch_sort, (4097, 3, 9000)),
    (OPS.test_layernorm_act, (300, 256, 100, True, 2)), (OPS.test_layernorm_act, (64, 64, 64, False, 0)),
    (OPS.test_segmax_and_adjoints, (3, 50, 64)), (OPS.test_segmax_nan_and_inf_follow_torch_max, (2, 1000, 130)),
    (OPS.test_colsum_tall, ()),
    (LOSS.test_weighted_l1_matches_reconstruction_loss, ((3, 7, 5),)), (LOSS.test_kld_matches_reference, ()),
    (LOSS.test_voxel_difference_bit_exact, ((3, 7, 5),)), (LOSS.test_voxel_difference_bit_exact, ((2049,),)),
    (LOSS.test_mean_sq_plain_and_row_weighted, ()),
    (LOSS.test_deepsdf_loss_is_the_sum_of_its_two_ops_bit_for_bit, (5000, 5000, 16, False)),
    (LOSS.test_deepsdf_loss_is_the_sum_of_its_two_ops_bit_for_bit, (1, 1, 1, True)),
    (LOSS.test_lerp_rows_bit_exact, ()), (LOSS.test_mean_difference_matches_torch, (128, 64)),
    (LOSS.test_mean_difference_matches_torch, (7, 0)), (LOSS.test_gradient_penalty_value_and_gradient, (5, (7, 3))),
    (LOSS.test_subsample2_bit_exact_and_adjoint, ()), (LOSS.test_fade_blend_first_and_second_order, (1, 0.3)),
    (LOSS.test_scatter_max_ragged, (1000, 7, 64, True)), (LOSS.test_scatter_max_ragged, (10, 12, 5, False)),
    (LOSS.test_head_dot_forward_and_backward, (6, 16, 1)), (LOSS.test_head_dot_forward_and_backward, (17, 8, 0)),
    (LOSS.test_head_dot_forward_and_backward, (3, 4, 2)), (LOSS.test_conv_head_node_matches_the_two_layer_composition, ()),
    (LOSS.test_bce_and_neg_mean_log_match_torch, (64,)), (LOSS.test_bce_and_neg_mean_log_match_torch, (1,)),
    (LOSS.test_vae_reparameterisation_matches_torch, ()),
    (M.test_sdf_generator_fused_vs_layerwise_and_oracle, ()), (M.test_gemm_nt_lnrelu_matches_torch, ()),
    (M.test_pointnet_select_matches_layerwise, (3, 1056)), (M.test_pointnet_select_matches_layerwise, (1, 32)),
    (M.test_rowdot_family_matches_torch_to_second_order, ()),
    (M.test_gather_rows_grouped_and_its_deterministic_adjoint, (2, 100, 300, 300)),
    (M.test_gather_rows_grouped_and_its_deterministic_adjoint, (1, 1, 5, 1)),
    (M.test_generator_fused_inference_matches_the_unfused_form, (5,)),
    (M.test_generator_forward_groups_equals_separate_evaluations, (3, 5)),
]


def _id(case):
    return "%s%s" % (case[0].__name__[5:], list(case[1]) if case[1] else "")


@pytest.mark.parametrize("case", BODIES, ids=_id)
def test_twin_body_under_poison(on_cpu, case):  # noqa: F811
    run_poisoned(case[0], *case[1])


def test_mesh_bodies_under_poison():
    for shape in ((6, 5, 7), (2, 2, 2), (1, 1, 1), (16, 16, 17)):
        assert shape in GR.MC_SHAPES
        run_poisoned(MESH.body_mc, "cpu", shape)
    run_poisoned(MESH.body_sampling, "cpu")


def test_evaluation_bodies_under_poison():
    for name in ("1x1", "64x33", "513x700"):
        run_poisoned(EV.check_matrix, name, "cpu")
        run_poisoned(EV.check_nearest, name, "cpu")
    run_poisoned(EV.check_ties, "cpu")
    run_poisoned(EV.check_non_finite, "cpu")
    run_poisoned(EV.check_histogram, "64x33", 5, "cpu")
    run_poisoned(EV.check_histogram, "1x1", 2, "cpu")
    run_poisoned(EV.check_set_scores, "64x33", "cpu")


def test_render_stage_bodies_under_poison(net, chairs_state, golden_latents):  # noqa: F811
    run_poisoned(RS.body_rays, "cpu")
    run_poisoned(RS.body_scene_and_shade, "cpu", 255, 1, False)
    run_poisoned(RS.body_scene_and_shade, "cpu", 1000, 6, True)
    run_poisoned(RS.body_get_shadows, net, chairs_state, golden_latents)
    run_poisoned(RS.body_no_hit_ground_is_inf, net, golden_latents)
