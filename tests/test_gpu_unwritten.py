"""GPU tier under poison: does every HIP kernel write all of its output, and does it read only scratch it wrote itself?

The value tests cannot tell a value a kernel wrote from one that was already there: outputs come from `torch.empty` (the caching
allocator recycles the block the previous kernel form just released — it holds the right answer) and scratch from `lib.workspace`
(cached per stream, never cleared).  Here (tests/poison.py) every such block starts as NaN (floats) / zero (integers and index scratch
on the GPU: an unwritten integer may be the next kernel's index and has to stay in bounds) and sits between canary bands.

  (a) the bodies of the existing GPU-tier tests run under poison — what they assert is unchanged — and the bands must be intact;
  (b) the raw entry points that return tensors: no NaN in a float output, integer outputs equal to the reference exactly;
  (c) every form runs twice on the same inputs, the poison renewed and the first run's blocks overwritten in between: the results are
      bit-identical.  That sees what (b) cannot: integer data, and a race on scratch.

EXEMPT from (c), by the only rule that allows it — the OUTPUT is accumulated with floating-point atomics, so the order of the additions
is the hardware's — one form, still compared with its reference:

    gather_rows backward (sg_scatter_add_rows)      csrc/elementwise.hip:279   atomicAdd(&table_grad[idx[i] * L + k], ...)

The other atomics of csrc/ order nothing that is observable: pointcloud.hip:180 (integer histogram counts), sdf_batch.hip:56 (integer
counts of a counting sort; positions come from a scan), elementwise.hip:184/186, sdfnet.hip:809 and losses.hip:314 (arrival tickets:
the LAST workgroup adds the partials in split order — not exempt), losses.hip:464/476 (atomicMax / atomicMin on integer images: order
free), raymarch.hip:83/203 (integer slot counters; the lists they fill are sorted or order-free downstream — run under (a), where
body_chunking repeats the march and compares), raymarch.hip:117 (an integer statistic), raymarch.hip:342/349 (integer atomicMin).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import poisoned, run_poisoned
import conv_patterns as GRIDS
import gemm_forms as GEMM
import evaluation_reference as ER
import test_evaluation as EV
import test_gpu_losses as LOSS
import test_gpu_mesh as GMESH
import test_gpu_modules as M
import test_gpu_ops as OPS
import test_render_stages as RS
from test_mesh import sphere_grid

pytestmark = pytest.mark.gpu
DEV = "cuda"

golden_latents = RS.golden_latents


@pytest.fixture(scope="module")
def net(chairs_state):
    from shapegan_amd.model.sdf_net import SDFNet
    n = SDFNet(device=DEV)
    n.load_state_dict(chairs_state)
    return n


def test_poison_on_the_device():
    """The helper on GPU tensors: transparent for shape / dtype / device / contiguity / alignment, NaN for floats, zero for integers and
    index scratch, 0xFF bytes (NaN as float and double) for float scratch, bands intact, nothing during stream capture."""
    import poison
    import shapegan_amd.lib as L
    src = torch.zeros(3, 5, device=DEV)
    with poisoned() as p:
        f, i, like = torch.empty((7, 3), device=DEV), torch.empty(9, dtype=torch.int32, device=DEV), torch.empty_like(src)
        for t, shape, dtype in ((f, (7, 3), torch.float32), (i, (9,), torch.int32), (like, (3, 5), torch.float32)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0
        assert bool(torch.isnan(f).all()) and bool(torch.isnan(like).all()) and bool((i == 0).all())
        ws, iws = L.workspace("splitk", 1000, src.device), L.workspace("mc", 300, src.device)
        assert ws.numel() == 1000 and ws.is_cuda and ws.data_ptr() % 16 == 0 and bool((ws == 0xFF).all()) and bool((iws == 0).all())
        assert bool(torch.isnan(ws[:992].view(torch.float32)).all()) and bool(torch.isnan(ws[:992].view(torch.float64)).all())
        p.check_canaries()
        p.records[0][0][poison.BAND + f.numel() * 4] = 0          # through the base buffer: one byte past the end of f
        with pytest.raises(poison.CanaryError):
            p.check_canaries()
        p.records[0][0][poison.BAND + f.numel() * 4] = poison.CANARY
        p.check_canaries()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            n = p.count
            captured = torch.empty(4, device=DEV).fill_(1.0)          # (the real allocator: nothing is recorded or filled)
            assert p.count == n and captured.is_cuda


# ---- (a) the existing bodies under poison ------------------------------------------------------------------------------------------
BODIES = [
    # conv forward: the forced gather / LDS-halo kernels (64- and 128-row tiles), the dispatching call
    (OPS.test_conv_fwd_halo_kernel, (1, 8, 32, 16)), (OPS.test_conv_fwd_halo_kernel, (2, 68, 130, 16)),
    (OPS.test_conv_fwd_halo_kernel, (1, 40, 64, 8)),
    (OPS.test_conv3d_fwd_dgrad_wgrad, (1, 2, 2, 2)), (OPS.test_conv3d_fwd_dgrad_wgrad, (2, 70, 130, 8)),
    (OPS.test_conv_dgrad_halo_kernel, (1, 32, 16, 8)), (OPS.test_conv_dgrad_halo_kernel, (3, 32, 64, 4)),
    (OPS.test_conv_dgrad_halo_kernel, (1, 64, 32, 16)),
    (OPS.test_conv_wgrad_halo_kernel, (1, 3, 32, 8)), (OPS.test_conv_wgrad_halo_kernel, (1, 3, 40, 4)),
    (OPS.test_conv_wgrad_halo_kernel, (9, 16, 130, 4)),
    (OPS.test_conv_wgrad_through_activation, (17, 24, 16, 2)),
    (OPS.test_producer_written_dy_images_equal_the_packing_pass, (37,)),
    (OPS.test_conv_transpose3d, (1, 5, 3, 3)), (OPS.test_conv_transpose3d, (70, 64, 1, 2)), (OPS.test_conv_transpose3d, (2, 3, 1, 12)),
    (OPS.test_conv_transpose3d_to_one_channel_random_shapes, ()),
    (OPS.test_conv_transpose3d_to_one_channel_streaming_kernel_random_shapes, ()),          # (all eight to1_pre forms)
    # the same families on grids of three different extents (tests/test_gpu_conv_grids.py)
    *GRIDS.DISPATCH_BODIES, *GRIDS.FORCED_BODIES,
    (OPS.test_linear_fwd_bwd, (5, 7, 3)), (OPS.test_linear_fwd_bwd, (200, 300, 130)), (OPS.test_linear_fwd_bwd, (4, 128, 256)),
    (OPS.test_linear_fwd_bwd, (16388, 384, 320)), (OPS.test_linear_fwd_bwd, (40004, 128, 100)),
    (OPS.test_gemm128_persistent_all_layouts, (70004, 256, 100)),
    (OPS.test_gemm_nt_bigk, (70, 130, 1000, 1003)), (OPS.test_gemm_nt_bigk, (256, 256, 31, 40)),
    # the GEMM family against float64 (tests/test_gpu_gemm_forms.py): one case per kernel kind, and the reductions
    *[(GEMM.body_gemm, (i,)) for i in GEMM.POISON_IDS], *[(GEMM.body_gemm_nt, (i,)) for i in GEMM.NT_POISON_IDS],
    (GEMM.body_rowsum, GEMM.ROWSUM_CASES[0]), (GEMM.body_rowsum_multi, GEMM.ROWSUM_MULTI_CASES[1]),
    (GEMM.body_segsum, GEMM.SEGSUM_CASES[1]), (GEMM.body_colsum, GEMM.COLSUM_CASES[3]),
    (OPS.test_colsum_tall, ()), (OPS.test_mean_reduction, ()), (OPS.test_gather_scatter_rows_bit_exact, ()),
    (OPS.test_batchnorm_train_fwd_bwd, (3, 7, 27)), (OPS.test_batchnorm_train_fwd_bwd, (4, 256, 1)),
    (OPS.test_batchnorm_train_fwd_bwd, (4, 24, 4096)),
    (OPS.test_layernorm_act, (7, 256, 7, 0, 2)), (OPS.test_layernorm_act, (300, 256, 100, 3, 2)),
    (OPS.test_segmax_and_adjoints, (1, 1, 7)), (OPS.test_segmax_and_adjoints, (2, 1000, 130)),
    (OPS.test_segmax_and_adjoints, (6, 32768, 512)),
    (LOSS.test_scatter_max_ragged, (10, 12, 5, False)), (LOSS.test_scatter_max_ragged, (1000, 7, 64, True)),
    (M.test_gather_rows_grouped_and_its_deterministic_adjoint, (1, 1, 5, 1)),
    (M.test_gather_rows_grouped_and_its_deterministic_adjoint, (2, 100, 300, 300)),
    (M.test_pointnet_select_matches_layerwise, (1, 32)), (M.test_pointnet_select_matches_layerwise, (3, 1056)),
    (OPS.test_sdfnet_points_mode, (1, 128)), (OPS.test_sdfnet_points_mode, (63, 128)), (OPS.test_sdfnet_points_mode, (130, 16)),
    (OPS.test_sdfnet_points_mode, (33100, 32)),
    (OPS.test_sdfnet_shapes_mode, (1, 37)), (OPS.test_sdfnet_shapes_mode, (5, 6656)),
    (OPS.test_sdfnet_segments_mode, (3, 129)), (OPS.test_sdfnet_segments_mode, (300, 1000)),
    (OPS.test_sdfnet_segments_mode, (7, 33100)),
    (M.test_sdf_generator_fused_vs_layerwise_and_oracle, ()),
    (OPS.test_sdf_batch_sort, (3, 1000, 1)), (OPS.test_sdf_batch_sort, (300, 7, 1000)), (OPS.test_sdf_batch_sort, (4097, 3, 9000)),
    (LOSS.test_deepsdf_loss_is_the_sum_of_its_two_ops_bit_for_bit, (1, 1, 1, True)),
    (LOSS.test_deepsdf_loss_is_the_sum_of_its_two_ops_bit_for_bit, (5000, 5000, 16, False)),
    (LOSS.test_bce_and_neg_mean_log_match_torch, (1,)), (LOSS.test_mean_sq_plain_and_row_weighted, ()),
    (LOSS.test_weighted_l1_matches_reconstruction_loss, ((1, 1),)), (LOSS.test_mean_difference_matches_torch, (1, 1)),
    (LOSS.test_mean_difference_matches_torch, (7, 0)), (LOSS.test_gradient_penalty_value_and_gradient, (5, (7, 3))),
    (LOSS.test_head_dot_forward_and_backward, (1, 4, 1)), (LOSS.test_head_dot_forward_and_backward, (5, 24, 2)),
    (LOSS.test_conv_head_node_matches_the_two_layer_composition, ()),
    # mesh, evaluation, render stages (the smallest cases of their files)
    (GMESH.test_gpu_matches_twin_single, ("noise0",)), (GMESH.test_gpu_marching_cubes_against_reference, ((2, 2, 2),)),
    (GMESH.test_gpu_marching_cubes_against_reference, ((6, 5, 7),)), (GMESH.test_gpu_marching_cubes_against_reference, ((1, 1, 1),)),
    (GMESH.test_gpu_surface_sampling_against_reference, ()), (GMESH.test_gpu_sample_surface_reproducible, ()),
    (EV.check_matrix, ("1x1", "cuda")), (EV.check_matrix, ("64x33", "cuda")), (EV.check_nearest, ("1x1", "cuda")),
    (EV.check_nearest, ("64x33", "cuda")), (EV.check_ties, ("cuda",)), (EV.check_non_finite, ("cuda",)),
    (EV.check_histogram, ("1x1", 2, "cuda")), (EV.check_histogram, ("64x33", 5, "cuda")), (EV.check_set_scores, ("64x33", "cuda")),
    (RS.body_rays, ("cuda",)), (RS.body_scene_and_shade, ("cuda", 255, 1, False)), (RS.body_scene_and_shade, ("cuda", 1000, 6, True)),
]


def _id(case):
    return "%s%s" % (case[0].__name__.replace("test_", ""), list(case[1]) if case[1] else "")


@pytest.mark.parametrize("case", BODIES, ids=_id)
def test_body_under_poison(case):
    run_poisoned(case[0], *case[1])


def test_render_march_bodies_under_poison(net, chairs_state, golden_latents):  # noqa: F811
    run_poisoned(RS.body_chunking, net, golden_latents, repeat=True)
    run_poisoned(RS.body_get_shadows, net, chairs_state, golden_latents)
    run_poisoned(RS.body_no_hit_ground_is_inf, net, golden_latents)


def test_conv_forward_workspace_is_in_use():
    """The dispatching forward at (2, 70, 130, 8) of the list above really takes scratch: its poisoned workspace is not a formality."""
    from shapegan_amd import lib as L
    assert L.load().sg_conv3d_k4s2p1_fwd_workspace_bytes(2, 70, 130, 4, 4, 4) > 0


# ---- (b) + (c): raw forms, twice, bit for bit -----------------------------------------------------------------------------------------
def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _check_outputs(outs, what):
    for k, t in enumerate(outs):
        if t.dtype.is_floating_point and bool(torch.isnan(t).any()):
            bad = torch.isnan(t).reshape(-1).nonzero().flatten()
            raise AssertionError("%s: output %d %s holds %d NaN (unwritten) element(s), first at flat index %d, last at %d" % (
                what, k, tuple(t.shape), bad.numel(), int(bad[0]), int(bad[-1])))


def run_form(make, check=None, exempt=None, what=""):
    """make() -> tensor(s), run twice under renewed poison; check(outputs on the CPU) is the comparison with the reference.
    exempt: the source line of the floating-point atomic that accumulates the output (the module docstring lists them)."""
    with poisoned() as p:
        first = _tuple(make())
        p.check_canaries()
        _check_outputs(first, what + " (first run)")
        kept = tuple(t.detach().to("cpu", copy=True) for t in first)
        del first
        p.renew()
        second = _tuple(make())
        p.check_canaries()
        _check_outputs(second, what + " (second run)")
        again = tuple(t.detach().to("cpu", copy=True) for t in second)
    if exempt is None:
        for k, (a, b) in enumerate(zip(kept, again)):
            assert a.dtype == b.dtype and torch.equal(a, b), "%s: output %d differs between two runs on the same inputs (%d elements)" % (
                what, k, int((a != b).sum()))
    if check is not None:
        check(kept)
        check(again)


def _lrelu(t):
    return F.leaky_relu(t, 0.2).float()


@pytest.mark.parametrize("N,Ci,Co,R", [(1, 8, 32, 16), (2, 68, 130, 16), (1, 40, 64, 8)])
def test_conv_forward_forms(N, Ci, Co, R):
    from shapegan_amd import ops
    torch.manual_seed(N + Ci + Co + R)
    x, w, b = torch.randn(N, Ci, R, R, R), torch.randn(Co, Ci, 4, 4, 4) / (Ci * 64) ** 0.5, torch.randn(Co)
    ref = _lrelu(F.conv3d(x.double(), w.double(), b.double(), stride=2, padding=1))
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    # (gather, halo, halo with 64- / 128-row tiles, 4 waves x 2 column tiles, no LDS cap)
    forms = [(0, 0), (1, 0)] + ([(1, 48), (1, 128), (1, 16), (1, 64)] if R // 2 >= 8 else [])
    for impl, debug in forms:
        what = "conv fwd impl %d debug %d" % (impl, debug)
        run_form(lambda: ops.conv_fwd_impl_raw(xg, wg, bg, 1, 0.2, impl=impl, debug=debug),
                 lambda o: OPS.close(o[0], ref, what=what), what=what)
    run_form(lambda: ops.conv_fwd_raw(xg, wg, bg, 1, 0.2), lambda o: OPS.close(o[0], ref, what="conv fwd"), what="conv fwd (dispatch)")


@pytest.mark.parametrize("N,Ci,Co,R", [(1, 2, 2, 2), (2, 70, 130, 8)])
def test_conv_dispatching_forms(N, Ci, Co, R):
    """Forward, input gradient and weight gradient as the dispatch rules pick them (ragged channel counts; a 1^3 output)."""
    from shapegan_amd import ops
    torch.manual_seed(N * 1000 + Ci * 10 + Co + R)
    x, w, b = torch.randn(N, Ci, R, R, R), torch.randn(Co, Ci, 4, 4, 4) / (Ci * 64) ** 0.5, torch.randn(Co)
    dy = torch.randn(N, Co, R // 2, R // 2, R // 2)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv3d(xr, wr, b.double(), stride=2, padding=1)
    y_ref.backward(dy.double())
    y_ref, dx_ref, dw_ref = y_ref.detach().float(), xr.grad.float(), wr.grad.float()
    xg, wg, bg, dyg = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    run_form(lambda: ops.conv_fwd_raw(xg, wg, bg), lambda o: OPS.close(o[0], y_ref, what="fwd"), what="conv fwd")
    run_form(lambda: ops.conv_dgrad_raw(dyg, wg, None, Ci), lambda o: OPS.close(o[0], dx_ref, what="dgrad"), what="conv dgrad")
    run_form(lambda: ops.conv_wgrad_raw(dyg, xg, Ci), lambda o: OPS.close(o[0], dw_ref, what="wgrad"), what="conv wgrad")


@pytest.mark.parametrize("N,Ci,Co,O", [(1, 32, 16, 8), (3, 32, 64, 4), (1, 64, 32, 16)])
def test_conv_dgrad_halo_forms(N, Ci, Co, O):
    from shapegan_amd import ops
    torch.manual_seed(N + Ci + Co + O)
    dy, w, b = torch.randn(N, Co, O, O, O), torch.randn(Co, Ci, 4, 4, 4) / (Co * 8) ** 0.5, torch.randn(Ci)
    ref = _lrelu(F.conv_transpose3d(dy.double(), w.double(), b.double(), stride=2, padding=1))
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    for ppw in (1, 2, 4, 8) if (Co // 16) % 2 == 0 else (1,):        # (several parities per workgroup: an even slab count only)
        impl = 1 if ppw == 1 else 1 + 4 * ppw
        what = "dgrad halo, %d parities per workgroup" % ppw
        run_form(lambda: ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, 1, 0.2, impl=impl), lambda o: OPS.close(o[0], ref, what=what), what=what)


@pytest.mark.parametrize("N,Ci,Co,ogrid", [(8, 72, 32, (4, 16, 32)), (255, 72, 32, (4, 4, 4))])
def test_conv_dgrad_halo_rows64_forms(N, Ci, Co, ogrid):
    """The 64-row kernels (conv_dgrad_halo_kernel<0> / <1>: what production takes at batch 64) with 4 (the dispatch rule), 1, 2, 4 and 8
    parities per workgroup; 72 input channels = a full row tile + 8 rows, 255 samples = a last workgroup with one sample."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY
    dy, w, b, ref = GRIDS.dgrad_inputs(N, Ci, Co, ogrid, "random", ACT_LEAKY)
    dyg, wg, bg = dy.cuda(), w.cuda(), b.cuda()
    for impl in (1, 3, 9, 17, 33):
        what = "dgrad halo, 64 rows, impl %d" % impl
        run_form(lambda: ops.conv_dgrad_halo_raw(dyg, wg, bg, Ci, ACT_LEAKY, 0.2, impl=impl), lambda o: OPS.close(o[0], ref, what=what), what=what)


@pytest.mark.parametrize("N,Ci,Co,O", [(1, 3, 32, 8), (1, 3, 40, 4), (9, 16, 130, 4)])
def test_conv_wgrad_halo_forms(N, Ci, Co, O):
    from shapegan_amd import ops
    torch.manual_seed(N + Ci + Co + O)
    x, dy = torch.randn(N, Ci, 2 * O, 2 * O, 2 * O), torch.randn(N, Co, O, O, O)
    w = torch.zeros(Co, Ci, 4, 4, 4, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), w, None, stride=2, padding=1).backward(dy.double())
    ref = w.grad.float()
    xg, dyg = x.cuda(), dy.cuda()
    run_form(lambda: ops.conv_wgrad_halo_raw(dyg, xg, Ci), lambda o: OPS.close(o[0], ref, what="wgrad halo"), what="wgrad halo")


def test_conv_wgrad_act_form():
    from shapegan_amd import ops
    N, Co, O, act = 17, 24, 16, 2
    torch.manual_seed(N + Co + O)
    x = torch.rand(N, 1, 2 * O, 2 * O, 2 * O) * 2 - 1
    w = (torch.randn(Co, 1, 4, 4, 4) * 0.2).requires_grad_(True)
    b = (torch.randn(Co) * 0.1).requires_grad_(True)
    pre = F.conv3d(x, w, b, stride=2, padding=1)
    y_ref = F.relu(pre)
    dy = torch.randn_like(y_ref)
    dy[pre.detach().abs() < 1e-5] = 0      # a pre-activation within rounding of the kink may take either branch on the GPU
    y_ref.backward(dy)
    dyg, yg, xg = dy.cuda(), y_ref.detach().cuda(), x.cuda()

    def check(o):
        OPS.close(o[0], w.grad, what="dw through activation")
        OPS.close(o[1], b.grad, what="db through activation")
    run_form(lambda: ops.conv_wgrad_act_raw(dyg, yg, xg, act, 0.2), check, what="wgrad_act")


@pytest.mark.parametrize("N,Ci,Co,R", [(1, 5, 3, 3), (70, 64, 1, 2), (2, 3, 1, 12)])
def test_conv_transpose_forms(N, Ci, Co, R):
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY, ACT_NONE, ACT_TANH
    torch.manual_seed(N + Ci + Co + R)
    x, w, b = torch.randn(N, Ci, R, R, R), torch.randn(Ci, Co, 4, 4, 4) / (Ci * 8) ** 0.5, torch.randn(Co)
    pre = F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    for act, fn in ((ACT_NONE, lambda t: t), (ACT_LEAKY, lambda t: F.leaky_relu(t, 0.2)), (ACT_TANH, torch.tanh)):
        ref, what = fn(pre).float(), "convT fwd act%d" % act
        with torch.no_grad():
            run_form(lambda: ops.conv_transpose3d_k4s2p1(xg, wg, bg, act, 0.2), lambda o: OPS.close(o[0], ref, what=what), what=what)


@pytest.mark.parametrize("N,C,R", [(5, 24, 6), (3, 7, 4), (9, 64, 16)])
def test_conv_transpose_to_one_channel_forms(N, C, R):
    """The dispatching entry (form 0) and every kernel form of sg_convT3d_k4s2p1_to1_pre_impl (3 and 4 were retired)."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY, ACT_TANH
    torch.manual_seed(N + R)
    x, w, b = torch.randn(N, C, R, R, R), torch.randn(C, 1, 4, 4, 4) / (C * 8) ** 0.5, torch.randn(1)
    scale, shift = torch.randn(C), torch.randn(C) * 0.3
    t = F.leaky_relu(x.double() * scale.double().view(1, C, 1, 1, 1) + shift.double().view(1, C, 1, 1, 1), 0.2)
    ref = torch.tanh(F.conv_transpose3d(t, w.double(), b.double(), stride=2, padding=1)).float()
    xg, wg, bg, sg, hg = x.cuda(), w.cuda(), b.cuda(), scale.cuda(), shift.cuda()
    for form in (0, 1, 2, 5, 6, 7, 8):
        what = "to1_pre form %d" % form
        run_form(lambda: ops.conv_transpose3d_to1_pre_raw(xg, sg, hg, ACT_LEAKY, 0.2, wg, bg, ACT_TANH, 0.0, form=form),
                 lambda o: OPS.close(o[0], ref, what=what), what=what)


@pytest.mark.parametrize("M_,N_,K_,layouts", [(5, 7, 3, 1), (200, 300, 130, 3), (4, 128, 256, 1), (16388, 384, 320, 3),
                                              (40004, 128, 100, 3), (70004, 256, 100, 3)])
def test_gemm_forms(M_, N_, K_, layouts):
    """sg_gemm in its operand layouts (forward / input gradient / weight gradient of a Linear layer), bias + LeakyReLU epilogue: the
    small-tile kernel, gemm128_kernel with a K split, and the persistent form (70004 rows: more than 512 tiles, ragged last tile)."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY
    torch.manual_seed(M_ + N_ + K_)
    a, b, bias = torch.randn(M_, K_), torch.randn(N_, K_) / K_ ** 0.5, torch.randn(N_)
    ref = _lrelu(a.double() @ b.double().t() + bias.double())
    ag, bg, biasg = a.cuda(), b.cuda(), bias.cuda()
    at, bt = a.t().contiguous().cuda(), b.t().contiguous().cuda()
    forms = [("A [M,K] x B [N,K]^T", lambda: ops.gemm_raw(ag, False, bg, True, bias_j=biasg, act=ACT_LEAKY, slope=0.2)),
             ("A [M,K] x B [K,N]", lambda: ops.gemm_raw(ag, False, bt, False, bias_j=biasg, act=ACT_LEAKY, slope=0.2)),
             ("A [K,M]^T x B [K,N]", lambda: ops.gemm_raw(at, True, bt, False, bias_j=biasg, act=ACT_LEAKY, slope=0.2))]
    for what, make in forms[:layouts]:
        run_form(make, lambda o: OPS.close(o[0], ref, what=what), what=what)
    if M_ >= 16388:      # the weight gradient of the same layer, dy^T [N,M] x a [M,K]: the long dimension is the reduction (K split)
        dy = torch.randn(M_, N_)
        ref_w = (dy.double().t() @ a.double()).float()
        dyg = dy.cuda()
        run_form(lambda: ops.gemm_raw(dyg, True, ag, False), lambda o: OPS.close(o[0], ref_w, what="dy^T x a"), what="dy [M,N]^T x A [M,K]")


@pytest.mark.parametrize("M_,N_,K_,lda", [(70, 130, 1000, 1003), (256, 256, 31, 40)])
def test_gemm_nt_forms(M_, N_, K_, lda):
    from shapegan_amd import ops
    torch.manual_seed(M_ + N_ + K_)
    a, b = torch.randn(M_, lda, device=DEV), torch.randn(N_, lda, device=DEV)
    want = (a[:, :K_].double() @ b[:, :K_].double().t()).cpu()

    def make():
        out = torch.empty((M_, N_), device=DEV)
        return ops.gemm_nt_raw(a, b, out, M_, N_, K_, lda, lda, N_)

    def check(o):
        assert float((o[0].double() - want).abs().max()) / float(want.abs().max()) < 2e-5
    run_form(make, check, what="gemm_nt")


def test_column_sums_and_mean_forms():
    from shapegan_amd import ops
    torch.manual_seed(5)
    for batch, rows, cols, ld in ((5, 3000, 70, 70), (3, 4099, 512, 516), (1, 7, 256, 256)):
        y = torch.randn(batch, rows, ld, device=DEV)
        want = y[:, :, :cols].double().sum(1).cpu().numpy()
        run_form(lambda: ops.colsum_tall_raw(y, batch, rows * ld, rows, cols, ld),
                 lambda o: np.testing.assert_allclose(o[0].numpy(), want, rtol=1e-5, atol=3e-3), what="colsum_tall %d x %d x %d" % (batch, rows, cols))
    g = torch.randn(100000, 256, device=DEV)
    want_g = g.double().sum(0).cpu().numpy()
    run_form(lambda: ops.ColSum.apply(g), lambda o: np.testing.assert_allclose(o[0].numpy(), want_g, rtol=1e-5, atol=2e-3), what="ColSum")
    for n in (64, 3_000_001):
        big = torch.randn(n) + 3
        bg = big.cuda()
        run_form(lambda: ops.mean(bg), lambda o: OPS.close(o[0], big.double().mean().float(), rtol=1e-5, atol=1e-7), what="mean of %d" % n)
    d = torch.randn(6, 24, 8, 8, 8)
    dg = d.cuda()
    run_form(lambda: ops.channel_sum_raw(dg), lambda o: OPS.close(o[0], d.double().sum((0, 2, 3, 4)).float(), rtol=1e-5), what="channel_sum")


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("per,C,S", [(3, 7, 27), (4, 256, 1), (4, 24, 4096)])
def test_batchnorm_grouped_forms(groups, per, C, S):
    """sg_bn_train_fwd_grouped and sg_bn_train_stats_grouped (ops.bn_train_stats_affine): `groups` independent batches stacked along
    dim 0, each against F.batch_norm in float64 on its own batch, the running statistics updated batch after batch.  Tolerance: the
    suite's fp32 bound of 1e-4 relative to the tensor's typical magnitude (OPS.close), 1e-3 where a channel has only per * S = 4 values
    — both as in test_batchnorm_train_fwd_bwd, whose reference is the same function."""
    from shapegan_amd import ops
    from shapegan_amd.lib import ACT_LEAKY
    torch.manual_seed(groups * 100 + per + C + S)
    shape = (groups * per, C, S) if S > 1 else (groups * per, C)
    x = torch.randn(shape) * 1.7 + 3.0
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    rm_r, rv_r = rm.double(), rv.double()
    ys, scales, shifts = [], [], []
    for g in range(groups):
        xb = x[g * per:(g + 1) * per].double()
        yb = F.batch_norm(xb, rm_r, rv_r, gamma.double(), beta.double(), True, 0.1, 1e-5)
        ys.append(F.leaky_relu(yb, 0.2))
        dims = (0, 2) if S > 1 else (0,)
        mean, var = xb.mean(dims), xb.var(dims, unbiased=False)
        scales.append(gamma.double() / torch.sqrt(var + 1e-5))
        shifts.append(beta.double() - mean * scales[-1])
    y_ref = torch.cat(ys).float()
    scale_ref, shift_ref = torch.stack(scales).float(), torch.stack(shifts).float()
    tol = 1e-3 if per * S <= 8 else OPS.RTOL
    xg, gg, bg = x.cuda(), gamma.cuda(), beta.cuda()

    def fwd():
        rm_g, rv_g, nbt = rm.cuda(), rv.cuda(), torch.zeros((), dtype=torch.long, device=DEV)
        y = ops.bn_train_fwd_grouped_raw(xg, gg, bg, rm_g, rv_g, nbt, 1e-5, 0.1, ACT_LEAKY, 0.2, groups)
        return y, rm_g, rv_g, nbt

    def stats():
        rm_g, rv_g, nbt = rm.cuda(), rv.cuda(), torch.zeros((), dtype=torch.long, device=DEV)
        scale, shift = ops.bn_train_stats_affine(xg, gg, bg, rm_g, rv_g, nbt, 1e-5, 0.1, groups=groups)
        return scale.reshape(groups, C), shift.reshape(groups, C), rm_g, rv_g, nbt

    def check_running(o):
        OPS.close(o[-3], rm_r.float(), rtol=tol, what="running_mean after %d groups" % groups)
        OPS.close(o[-2], rv_r.float(), rtol=tol, what="running_var after %d groups" % groups)
        assert int(o[-1]) == groups

    def check_fwd(o):
        OPS.close(o[0], y_ref, rtol=tol, what="grouped bn fwd")
        check_running(o)

    def check_stats(o):
        OPS.close(o[0], scale_ref, rtol=tol, what="grouped bn scale")
        OPS.close(o[1], shift_ref, rtol=tol, what="grouped bn shift")
        check_running(o)
    run_form(fwd, check_fwd, what="bn_train_fwd_grouped, %d groups" % groups)
    run_form(stats, check_stats, what="bn_train_stats_affine, %d groups" % groups)


@pytest.mark.parametrize("B,P,C", [(1, 1, 7), (2, 1000, 130), (6, 32768, 512)])
def test_segmax_forms(B, P, C):
    from shapegan_amd import ops
    torch.manual_seed(B * P + C)
    x = torch.randn(B, P, C)
    if P > 4:
        x[:, 3] = x[:, 1]                      # exact ties: the first occurrence must win
    want_v = x.max(dim=-2)[0]
    first = (x == want_v.unsqueeze(1)).float().argmax(dim=1)
    xg = x.cuda()

    def check(o):
        assert torch.equal(o[0], want_v) and o[1].dtype == torch.int32 and torch.equal(o[1].long(), first)
    run_form(lambda: ops.SegMax.apply(xg), check, what="segmax")
    idx, dy, u = first.int().cuda(), torch.randn(B, C, device=DEV), torch.randn(B, P, C, device=DEV)
    ref_s = torch.zeros(B, P, C).scatter_(1, first.unsqueeze(1), dy.cpu().unsqueeze(1))
    ref_g = u.cpu().gather(1, first.unsqueeze(1)).squeeze(1)
    run_form(lambda: ops.SegMaxScatter.apply(dy, idx, P), lambda o: torch.testing.assert_close(o[0], ref_s, rtol=0, atol=0), what="segmax scatter")
    run_form(lambda: ops.SegMaxGather.apply(u, idx), lambda o: torch.testing.assert_close(o[0], ref_g, rtol=0, atol=0), what="segmax gather")


@pytest.mark.parametrize("N,B,C,sorted_batch", [(10, 12, 5, False), (1000, 7, 64, True)])
def test_scatter_max_forms(N, B, C, sorted_batch):
    from shapegan_amd import ops
    torch.manual_seed(N + B + C)
    x = torch.randn(N, C)
    batch = torch.randint(0, B, (N,))
    if sorted_batch:
        batch = torch.sort(batch)[0]
    want = torch.zeros(B, C)
    arg = torch.full((B, C), -1, dtype=torch.long)
    for b in range(B):
        rows = (batch == b).nonzero().flatten()
        if rows.numel():
            v, i = x[rows].max(0)
            want[b], arg[b] = v, rows[(x[rows] == v).float().argmax(0)]
    xg, bg = x.cuda(), batch.cuda()

    def check(o):
        assert torch.equal(o[0], want) and torch.equal(o[1].long(), arg)
    run_form(lambda: ops.ScatterMax.apply(xg, bg, B), check, what="scatter_max")


@pytest.mark.parametrize("B,C,P,U", [(1, 1, 5, 1), (2, 100, 300, 300)])
def test_gather_rows_grouped_forms(B, C, P, U):
    from shapegan_amd import ops
    torch.manual_seed(B + C + P + U)
    x = torch.randn(B * P, 8)
    rows = (torch.randint(0, min(U, P), (B, C)) + torch.arange(B).view(B, 1) * P).reshape(-1)
    xg, rg = x.cuda().requires_grad_(True), rows.cuda()
    g = torch.randn(B * C, 8)
    gg = g.cuda()
    want_dx = torch.zeros_like(x).index_add_(0, rows, g)

    def make():
        out = ops.gather_rows_grouped(xg, rg, C)
        (dx,) = torch.autograd.grad(out, xg, gg)
        return out, dx

    def check(o):
        assert torch.equal(o[0], x[rows])
        OPS.close(o[1], want_dx, rtol=1e-5, atol=1e-5, what="deterministic adjoint of the grouped gather")
    run_form(make, check, what="gather_rows_grouped")


def test_gather_rows_and_its_atomic_adjoint():
    """The one exempt form: sg_scatter_add_rows accumulates the table gradient with float atomicAdd (csrc/elementwise.hip:279), so two runs
    may differ in the last bits; both are compared with the reference, and the gather itself (index work) is not exempt."""
    from shapegan_amd import ops
    torch.manual_seed(5)
    table, idx, g = torch.randn(37, 128), torch.randint(0, 37, (1000,)), torch.randn(1000, 128)
    tg, ig, gg = table.cuda().requires_grad_(True), idx.cuda(), g.cuda()
    ref = torch.zeros_like(table).index_add_(0, idx, g)
    run_form(lambda: ops.gather_rows(tg.detach(), ig), lambda o: torch.testing.assert_close(o[0], table[idx], rtol=0, atol=0), what="gather_rows")
    run_form(lambda: torch.autograd.grad(ops.gather_rows(tg, ig), tg, gg), lambda o: OPS.close(o[0], ref, rtol=1e-5, atol=1e-5),
             exempt="csrc/elementwise.hip:279", what="gather_rows backward")


@pytest.mark.parametrize("B,P", [(1, 32), (3, 1056)])
def test_pointnet_select_forms(B, P):
    from shapegan_amd import ops
    from shapegan_amd.model.point_sdf_net import PointNet, _run_mlp
    torch.manual_seed(94)
    D = PointNet(out_channels=1).to(DEV)
    x = torch.cat([torch.rand(B, P, 3) * 2 - 1, torch.rand(B, P, 1) * 0.2 - 0.1], -1).cuda()
    lins = [m for m in D.nn1 if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        h = _run_mlp(D.nn1, x.reshape(-1, 4)).reshape(B, P, 512).cpu()
    ref = h.max(dim=1)[0]

    def check(o):
        OPS.close(o[0], ref, rtol=1e-5, atol=1e-6, what="pointnet_select maxima")
        assert o[1].dtype == torch.int32 and int(o[1].min()) >= 0 and int(o[1].max()) < P
        OPS.close(h.gather(1, o[1].long().unsqueeze(1)).squeeze(1), ref, rtol=1e-5, atol=1e-6, what="value at the selected point")
    run_form(lambda: ops.pointnet_select(D._pack, x, [l.weight for l in lins], [l.bias for l in lins]), check, what="pointnet_select")


@pytest.mark.parametrize("S,pc,N", [(3, 1000, 1), (300, 7, 1000), (4097, 3, 9000)])
def test_sdf_batch_sort_forms(S, pc, N):
    from shapegan_amd import ops
    torch.manual_seed(S + N)
    points, sdf, idx = torch.rand(S * pc, 3) * 2 - 1, torch.rand(S * pc) * 0.2 - 0.1, torch.randint(0, S * pc, (N,))
    if S == 300:
        idx = (torch.randint(0, S // 2, (N,)) * 2) * pc + torch.randint(0, pc, (N,))      # odd shapes are absent
    shape = torch.div(idx, pc, rounding_mode="floor")
    order = torch.sort(shape, stable=True)[1]
    cnt = torch.bincount(shape, minlength=S)
    ig, pg, sg = idx.cuda(), points.cuda(), sdf.cuda()

    def check(o):
        bp, bs, sid, seg_off, counts = o
        assert torch.equal(bp, points[idx[order]]) and torch.equal(bs, sdf[idx[order]])
        assert sid.dtype == torch.int32 and torch.equal(sid.long(), shape[order]) and torch.equal(counts, cnt.float())
        assert seg_off.dtype == torch.int64 and int(seg_off[0]) == 0 and torch.equal(seg_off[1:], torch.cumsum(cnt, 0))
    run_form(lambda: ops.sdf_batch_sort(ig, pc, S, pg, sg), check, what="sdf_batch_sort")
    ops.check_batch_indices()


def _sdf_grads(out, dy, inputs, net):
    params = [p for p in net.parameters()]
    return (out.detach(),) + torch.autograd.grad(out, list(inputs) + params, dy)


@pytest.mark.parametrize("N,latent", [(1, 128), (63, 128), (130, 16), (33100, 32)])
def test_sdfnet_points_forms(N, latent):
    """Forward and the whole backward (input, latent and parameter gradients: the arrival-ticket reductions add in split order and are
    NOT exempt) twice; the values against the oracle are test_sdfnet_points_mode's, run under poison in (a)."""
    net = OPS._sdf_state(8, latent)
    torch.manual_seed(N)
    pts, lat, dy = (torch.rand(N, 3) * 2 - 1).cuda(), (torch.randn(N, latent) * 0.5).cuda(), torch.randn(N).cuda()

    def make():
        pg, lg = pts.clone().requires_grad_(True), lat.clone().requires_grad_(True)
        return _sdf_grads(net(pg, lg).reshape(-1), dy, (pg, lg), net)
    run_form(make, what="sdfnet points")


@pytest.mark.parametrize("S,pps", [(1, 37), (5, 6656)])
def test_sdfnet_shapes_forms(S, pps):
    net = OPS._sdf_state(9)
    torch.manual_seed(S * pps)
    pts, z, dy = (torch.rand(S * pps, 3) * 2 - 1).cuda(), torch.randn(S, 128).cuda(), torch.randn(S * pps).cuda()

    def make():
        pg, zg = pts.clone().requires_grad_(True), z.clone().requires_grad_(True)
        return _sdf_grads(net.forward_shapes(pg, zg, pps), dy, (pg, zg), net)
    run_form(make, what="sdfnet shapes")


@pytest.mark.parametrize("S,N", [(3, 129), (300, 1000), (7, 33100)])
def test_sdfnet_segments_forms(S, N):
    net = OPS._sdf_state(10)
    torch.manual_seed(S + N)
    table = (torch.randn(S, 128) * 0.5).cuda()
    sid = torch.sort(torch.randint(0, S, (N,)))[0]
    if S == 300:
        sid = torch.sort(torch.randint(0, S // 2, (N,)) * 2)[0]          # odd shapes are absent
    seg_off = torch.zeros(S + 1, dtype=torch.int64)
    seg_off[1:] = torch.cumsum(torch.bincount(sid, minlength=S), 0)
    pts, dy, sid_g, seg_g = (torch.rand(N, 3) * 2 - 1).cuda(), torch.randn(N).cuda(), sid.cuda().int(), seg_off.cuda()

    def make():
        tg = table.clone().requires_grad_(True)
        return _sdf_grads(net.forward_segments(pts, tg, sid_g, seg_g), dy, (tg,), net)
    run_form(make, what="sdfnet segments")


def test_loss_forms():
    """Each fused loss at its smallest parameters and one size with more than one block: value and gradients, twice."""
    from shapegan_amd import ops
    torch.manual_seed(3)

    def with_grad(fn, *tensors):
        def make():
            leaves = [t.clone().requires_grad_(True) for t in tensors]
            loss = fn(*leaves)
            return (loss.detach(),) + torch.autograd.grad(loss, leaves)
        return make

    for n, rows, L in ((1, 1, 1), (5000, 50, 16)):
        out, target, z = torch.randn(n).cuda() * 0.1, torch.randn(n).cuda() * 0.1, torch.randn(rows, L).cuda()
        weight = (torch.rand(rows) * 3).cuda()
        ref = (out.double() - target.double()).abs().mean() + (z.double().pow(2).sum(1) * weight.double()).sum() / n

        def check(o, ref=ref):
            OPS.close(o[0], ref.float().cpu(), rtol=1e-5, what="deepsdf loss")
        run_form(with_grad(lambda o, zz: ops.deepsdf_loss(o, target, zz, weight, float(n)), out, z), check, what="deepsdf n=%d" % n)
        x = torch.randn(rows, L).cuda()
        run_form(with_grad(lambda t: ops.mean_sq(t), x), lambda o, x=x: OPS.close(o[0], x.double().pow(2).mean().float().cpu(), rtol=1e-5),
                 what="mean_sq")
        p = (torch.rand(n) * 0.98 + 0.01).cuda()
        run_form(with_grad(lambda t: ops.bce_const(t, 1.0), p), lambda o, p=p: OPS.close(o[0], (-p.double().log()).mean().float().cpu(), rtol=1e-5),
                 what="bce")
        run_form(with_grad(lambda t: ops.neg_mean_log(t), p), lambda o, p=p: OPS.close(o[0], (-p.double().log()).mean().float().cpu(), rtol=1e-5),
                 what="neg_mean_log")
        o3, t3 = torch.randn(n, 4, 4).cuda(), (torch.randn(n, 4, 4).cuda() > 0).float() * 2 - 1
        run_form(with_grad(lambda t: ops.weighted_l1(t, t3, 1.0), o3), lambda o, a=o3, b=t3: OPS.close(o[0], (a.double() - b.double()).abs().mean().float().cpu(), rtol=1e-5),
                 what="weighted_l1")
        run_form(with_grad(lambda t: ops.mean_difference(t, (n + 1) // 2), out) if n > 1 else with_grad(lambda t: ops.mean(t), out), what="mean difference")
    gr = torch.randn(5, 7, 3).cuda()
    ref_gp = ((gr.double().reshape(5, -1).norm(dim=1) - 1) ** 2).mean() * 10.0
    run_form(with_grad(lambda t: ops.gradient_penalty(t, 10.0), gr), lambda o: OPS.close(o[0], ref_gp.float().cpu(), rtol=1e-5), what="gradient penalty")


@pytest.mark.parametrize("N,C,act", [(1, 4, 1), (5, 24, 2)])
def test_head_forms(N, C, act):
    """The critic's tail (ops.conv_head: Conv3d k4s2p1 -> activation -> Conv3d(C -> 1) over the 4^3 grid): value and gradients, twice."""
    from shapegan_amd import ops
    torch.manual_seed(N + C)
    Ci = 8
    x, w, b = torch.randn(N, Ci, 8, 8, 8).cuda(), (torch.randn(C, Ci, 4, 4, 4) * 0.05).cuda(), torch.randn(C).cuda()
    wh, bh = (torch.randn(1, C, 4, 4, 4) * 0.05).cuda(), torch.randn(1).cuda()
    fn = (lambda t: F.leaky_relu(t, 0.2)) if act == 1 else F.relu
    ref = F.conv3d(fn(F.conv3d(x.double(), w.double(), b.double(), stride=2, padding=1)), wh.double(), bh.double()).reshape(N).float().cpu()
    g = torch.randn(N).cuda()

    def make():
        leaves = [t.clone().requires_grad_(True) for t in (x, w, b, wh, bh)]
        y = ops.conv_head(leaves[0], leaves[1], leaves[2], act, 0.2, leaves[3], leaves[4]).reshape(N)
        return (y.detach(),) + torch.autograd.grad(y, leaves, g)
    run_form(make, lambda o: OPS.close(o[0], ref, what="conv_head"), what="conv_head")


def test_mesh_forms():
    """Marching cubes (offsets and faces are integers: equal to the twin exactly) and surface sampling, twice."""
    from shapegan_amd.mesh import marching_cubes, sample_packed
    grids = torch.stack([torch.from_numpy(sphere_grid(16, 0.6)), torch.rand((16, 16, 16), generator=torch.Generator().manual_seed(1)) * 2 - 1,
                         torch.ones(16, 16, 16)])
    kw = dict(level=0.0, spacing=(2 / 15, 0.07, 0.05), origin=(-1, -0.5, 0.25))
    cpu = marching_cubes(grids, **kw)
    gg = grids.cuda()

    def mc():
        m = marching_cubes(gg, **kw)
        return m.vertices, m.normals, m.faces, m.vert_offsets, m.tri_offsets

    def check(o):
        assert torch.equal(o[2], cpu.faces) and torch.equal(o[3], cpu.vert_offsets) and torch.equal(o[4], cpu.tri_offsets)
        torch.testing.assert_close(o[0], cpu.vertices, rtol=0, atol=1e-6)
        torch.testing.assert_close(o[1], cpu.normals, rtol=0, atol=1e-6)
    run_form(mc, check, what="marching cubes")
    gpu = marching_cubes(gg, **kw)
    u = torch.rand((3, 5000, 3), generator=torch.Generator().manual_seed(11))
    ug = u.cuda()
    pc, ec = sample_packed(cpu.vertices, cpu.faces, cpu.vert_offsets, cpu.tri_offsets, u)

    def check_s(o):
        assert o[1].tolist() == ec.tolist() == [0, 0, 1] and bool((o[0][2] == 0).all())
        # (tree against sequential sum of the cumulative areas: a sample within rounding of a triangle boundary may pick the neighbour)
        assert float(((o[0] - pc).abs().amax(dim=2) > 1e-5).float().mean()) < 1e-3
    run_form(lambda: sample_packed(gpu.vertices, gpu.faces, gpu.vert_offsets, gpu.tri_offsets, ug), check_s, what="mesh sampling")


@pytest.mark.parametrize("name", ["1x1", "64x33", "513x700"])
def test_evaluation_forms(name):
    """Chamfer matrices, nearest neighbours (indices: equal to the twin exactly, as include/shapegan_hip.h promises) and histograms."""
    from shapegan_amd import evaluation as E
    a, b = ER.case_sets(name)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    want = E.chamfer_matrix(ta, tb)
    run_form(lambda: E.chamfer_matrix(ta.cuda(), tb.cuda()), lambda o: [np.testing.assert_array_equal(x.numpy(), y.numpy()) for x, y in zip(o, want)],
             what="chamfer_matrix")
    pa, pb = (torch.from_numpy(x) for x in EV.all_pairs(a, b))
    want_n = E.nearest_neighbours(pa, pb)
    run_form(lambda: E.nearest_neighbours(pa.cuda(), pb.cuda()),
             lambda o: [np.testing.assert_array_equal(x.numpy(), y.numpy()) for x, y in zip(o, want_n)], what="nearest_neighbours")
    want_h = E.occupancy_histogram(ta, 7)
    run_form(lambda: E.occupancy_histogram(ta.cuda(), 7), lambda o: np.testing.assert_array_equal(o[0].numpy(), want_h.numpy()), what="histogram")


@pytest.mark.parametrize("R,C,rps,tail,act", [(7, 256, 7, 0, 2), (300, 256, 100, 3, 2)])
def test_layernorm_forms(R, C, rps, tail, act):
    """y = act(LN(x + zrow[r // rps])) (+ tail columns) and its backward (two-pass dgamma / dbeta through the `layernorm` scratch) against
    torch in float64, at test_layernorm_act's bound (2e-5 of the tensor's largest magnitude), twice."""
    from shapegan_amd import ops
    torch.manual_seed(R + C)
    x, zb = torch.randn(R, C) * 2 + 0.5, torch.randn(R // rps, C)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    t = torch.randn(R, tail) if tail else None
    w = torch.randn(R, C + tail)
    leaves = [v.double().requires_grad_(True) for v in (x, zb, gamma, beta)]
    y = F.relu(F.layer_norm(leaves[0] + leaves[1].repeat_interleave(rps, 0), (C,), leaves[2], leaves[3], 1e-5))
    y = torch.cat([y, t.double()], 1) if tail else y
    want = (y.detach(),) + torch.autograd.grad(y, leaves, w.double())
    xg, zg, gg, bg, wg, tg = x.to(DEV), zb.to(DEV), gamma.to(DEV), beta.to(DEV), w.to(DEV), None if t is None else t.to(DEV)

    def make():
        ls = [v.clone().requires_grad_(True) for v in (xg, zg, gg, bg)]
        out = ops.layernorm_act(ls[0], ls[1], rps, ls[2], ls[3], 1e-5, act, tg)
        return (out.detach(),) + torch.autograd.grad(out, ls, wg)

    def check(o):
        for name, a, e in zip(("y", "dx", "dz", "dgamma", "dbeta"), o, want):
            assert float((a.double() - e).abs().max()) / (float(e.abs().max()) + 1e-12) < 2e-5, name
    run_form(make, check, what="layernorm_act")
