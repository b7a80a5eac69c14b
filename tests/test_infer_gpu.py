"""The forward nobody differentiates (GPU): the persistent GEMM's fc1 call with a single output, devias_encoder_block_infer against the training forward and
against the per-kernel sequence of the teacher, the student's and the teacher's forward with the switch on and off, and the two evaluation entry points of the
engine on real models.  Everything is compared BITWISE: the new path runs the same launches on the same operands."""
import ctypes

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ 1. GEMM: bias + GELU, one output
@pytest.mark.parametrize("M,N,K", [(256 * 70, 1024, 128), (256 * 99, 768, 768)])
def test_gemm_gelu_single_output_is_bitwise_the_generic_and_the_two_output_form(M, N, K):
    """fc1 as the forward-only block calls it: the C stored is that of the two-output call, under either setting of gemm_epi_spec, on the queues and on static lists
    with the tail in thirds.  (The call has no compile-time epilogue of its own -- DESIGN.md section 5 -- and runs the generic form; the test holds either way, and the
    float64 bound of this C is the existing gelu_aux cases'.)"""
    from devias_amd import ops as o
    A, B, bias, _res = kb.gemm_inputs(M, N, K, BF, spread=6, seed=400, device=DEV)

    def run(**kw):
        o.counters(reset=True)
        c = o.gemm(A, B, bias=bias, act=o.ACT_GELU, **kw)
        torch.cuda.synchronize()
        return c, o.counters()

    for dyn in (1, 0):
        with o.options(gemm_persistent=1, gemm_dynamic=dyn, gemm_tail_split=3):
            with o.options(gemm_epi_spec=1):
                c1, n1 = run()
                aux = torch.empty(M, N, dtype=BF, device=DEV)
                c2, n2 = run(aux_out=aux)
            with o.options(gemm_epi_spec=0):
                c0, n0 = run()
        for n in (n1, n2, n0):
            assert n["gemm256p"] == 1 and n["gemm256"] == 0 and n["gemm256w"] == 0 and n["gemm256d"] == int(bool(dyn) and K >= 128), (dyn, n)
        assert torch.isfinite(c1.float()).all()
        assert torch.equal(c1, c0), f"dyn={dyn}: specialised != generic"
        assert torch.equal(c1, c2), f"dyn={dyn}: one output != two outputs"


# ------------------------------------------------------------------------------------------------ 2 / 3. the region through ctypes
def _block_params(D, hid, dtype, seed, qscaled):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)  # noqa: E731
    p = {"n1w": 1.0 + r(D, k=0.1), "n1b": r(D, k=0.1), "n2w": 1.0 + r(D, k=0.1), "n2b": r(D, k=0.1),
         "Wqkv": r(3 * D, D, k=D ** -0.5).to(dtype), "Wp": r(D, D, k=D ** -0.5).to(dtype), "W1": r(hid, D, k=D ** -0.5).to(dtype), "W2": r(D, hid, k=hid ** -0.5).to(dtype),
         "qkv_bias": r(3 * D, k=0.1), "pb": r(D, k=0.1), "b1": r(hid, k=0.1), "b2": r(D, k=0.1)}
    if qscaled:          # any second copy will do here: both entry points must read IT, and say so to the attention
        p["WqkvS"] = (p["Wqkv"].float() * 0.18).to(dtype)
        p["qkv_biasS"] = p["qkv_bias"] * 0.18
    return {k: v.to(DEV).contiguous() for k, v in p.items()}


def _args(p, B, N, D, H, hid, dtype):
    from devias_amd import _lib
    a = _lib.BlockArgs()
    a.B, a.N, a.D, a.H, a.hidden, a.dtype, a.eps = B, N, D, H, hid, (_lib.BF16 if dtype == BF else _lib.F32), 1e-6
    for k, v in p.items():
        setattr(a, k, v.data_ptr())
    return a


def _infer(p, x, B, N, H, hid, fill):
    """devias_encoder_block_infer on a workspace of exactly the queried size, pre-filled with `fill` bytes -> (x2, counters)"""
    from devias_amd import _lib, ops
    lib = _lib.load()
    rows, D = x.shape
    a = _args(p, B, N, D, H, hid, x.dtype)
    need = lib.devias_encoder_block_infer_workspace_bytes(B, N, rows, D, H, hid, a.dtype)
    ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    a.ws, a.ws_bytes = ws.data_ptr(), need
    x2 = torch.full_like(x.view(torch.uint8), fill).view(x.dtype).view(rows, D)
    torch.cuda.synchronize()
    ops.counters(reset=True)
    _lib.check(lib.devias_encoder_block_infer(ctypes.byref(a), x.data_ptr(), x2.data_ptr(), rows, ops._stream()), "devias_encoder_block_infer")
    torch.cuda.synchronize()
    return x2, ops.counters()


def _train_fwd(p, x, B, N, H, hid):
    from devias_amd import _lib, ops
    lib = _lib.load()
    M, D = x.shape
    a = _args(p, B, N, D, H, hid, x.dtype)
    save = torch.empty((lib.devias_encoder_block_save_bytes(B, N, D, H, hid, a.dtype),), dtype=torch.uint8, device=DEV)
    ws = torch.empty((lib.devias_encoder_block_workspace_bytes(B, N, D, H, hid, a.dtype),), dtype=torch.uint8, device=DEV)
    a.save, a.ws, a.ws_bytes = save.data_ptr(), ws.data_ptr(), ws.numel()
    x2 = torch.empty_like(x)
    torch.cuda.synchronize()
    ops.counters(reset=True)
    _lib.check(lib.devias_encoder_block_fwd(ctypes.byref(a), x.data_ptr(), x2.data_ptr(), ops._stream()), "devias_encoder_block_fwd")
    torch.cuda.synchronize()
    return x2, ops.counters()


def _x(rows, D, dtype, real=None, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if real is not None:
        x[real:] = 0.0
    return x.to(dtype).to(DEV).contiguous()


@pytest.mark.parametrize("case", ["bf16", "bf16_qscaled", "fp32"])
def test_region_is_bitwise_the_training_forward(case):
    """bf16: M = 98 x 256 rows; qkv (294 tiles) and fc1 (392 tiles) exceed one round on 256 CUs -- the persistent kernel serves them --,
    proj and fc2 (98 tiles each) take the one-tile-per-workgroup kernel, as in training"""
    dtype = F32 if case == "fp32" else BF
    B, N, D, H, hid = (2, 196, 128, 2, 512) if case == "fp32" else (16, 1568, 256, 4, 1024)
    p = _block_params(D, hid, dtype, 5, case == "bf16_qscaled")
    x = _x(B * N, D, dtype)
    ref, cref = _train_fwd(p, x, B, N, H, hid)
    assert torch.isfinite(ref.float()).all()
    outs = []
    for fill in (0xFF, 0x00):
        x2, cnt = _infer(p, x, B, N, H, hid, fill)
        assert cnt.pop("block_infer") == 1 and cref["block_infer"] == 0
        assert cnt == {k: v for k, v in cref.items() if k != "block_infer"}, (cnt, cref)          # every GEMM and attention family: the same launches
        assert torch.equal(x2, ref), f"{case}, workspace filled with {fill:#x}: x2 differs from the training forward's"
        outs.append(x2)
    assert torch.equal(outs[0], outs[1])
    if dtype == BF:
        assert cref["gemm256p"] == 2 and cref["gemm256"] == 2 and cref["mhsa_fwd_bf16"] == 1 and cref["mhsa_qpre"] == int(case == "bf16_qscaled"), cref
    else:
        assert cref["gemm128_f32"] == 4 and cref["mhsa_fwd_f32"] == 1, cref


@pytest.mark.parametrize("dtype", [BF, F32])
def test_region_ragged_rows_match_the_teachers_kernel_sequence(dtype):
    """B = 3 clips of 197 tokens in 768 rows (591 real): LayerNorm and the GEMMs over all rows, the attention over the real ones, the pad rows of o zeroed by the call"""
    from devias_amd import ops
    B, N, D, H, hid, rows = 3, 197, 128, 2, 512, 768
    M = B * N
    p = _block_params(D, hid, dtype, 6, False)
    h = _x(rows, D, dtype, real=M)
    # the per-kernel sequence of modeling_finetune.VisionTransformer.forward_features on the same padded buffers
    o = torch.zeros((rows, D), dtype=dtype, device=DEV)
    u, _, _ = ops.layernorm_fwd(h, p["n1w"], p["n1b"], 1e-6)
    qkv = ops.gemm(u, p["Wqkv"], bias=p["qkv_bias"])
    ops.mhsa_fwd(qkv[:M], B, N, H, 64 ** -0.5, out=o[:M])
    h1 = ops.gemm(o, p["Wp"], bias=p["pb"], res=h)
    u2, _, _ = ops.layernorm_fwd(h1, p["n2w"], p["n2b"], 1e-6)
    act = ops.gemm(u2, p["W1"], bias=p["b1"], act=ops.ACT_GELU)
    ref = ops.gemm(act, p["W2"], bias=p["b2"], res=h1)
    torch.cuda.synchronize()
    assert torch.isfinite(ref.float()).all()
    outs = []
    for fill in (0xFF, 0x00):
        x2, cnt = _infer(p, h, B, N, H, hid, fill)
        assert cnt["block_infer"] == 1
        assert torch.equal(x2[:M], ref[:M]), f"workspace filled with {fill:#x}: real rows differ"
        assert torch.isfinite(x2[M:].float()).all()
        assert torch.equal(x2[M:], ref[M:])          # (pad rows of x2 are a function of the pad rows of x: the per-kernel sequence's too)
        outs.append(x2)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 4. student
def _student(dtype, **kw):
    from functools import partial
    from devias_amd import synth
    from devias_amd.modeling_slot import VisionTransformer
    m = VisionTransformer(img_size=64, patch_size=16, embed_dim=384, depth=2, num_heads=6, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                          num_classes=10, all_frames=4, tubelet_size=2, init_scale=1.0, num_latents=2, head_type="linear", slot_matching_method="matching",
                          agg_weights_tie=True, agg_depth=2, num_scene_classes=6, compute_dtype=dtype, **kw)
    with torch.no_grad():
        synth.fill_module_(m, seed=0)
    return m.cuda().eval()


def _teacher(dtype, img_size, **kw):
    """vit_base_patch16_224's settings at embed_dim 128, depth 2, 2 heads (the factory itself fixes 768 / 12 / 12)"""
    from functools import partial
    from devias_amd import synth
    from devias_amd.modeling_finetune import VisionTransformer
    m = VisionTransformer(patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                          all_frames=4, img_size=img_size, use_mean_pooling=False, init_scale=1.0, compute_dtype=dtype, **kw)
    with torch.no_grad():
        synth.fill_module_(m, seed=1)
    return m.cuda().eval()


def _flat(out):
    res = []
    for t in out:
        res += _flat(t) if isinstance(t, (tuple, list)) else [t]
    return res


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import devias_amd.modeling_slot as ms
        self.old, ms._INFER = ms._INFER, self.on

    def __exit__(self, *exc):
        import devias_amd.modeling_slot as ms
        ms._INFER = self.old


def _counted(fn):
    from devias_amd import ops
    ops.counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, ops.counters()["block_infer"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_student_no_grad_forward_is_bitwise_equal_and_training_does_not_go_near_it(dtype):
    from devias_amd import synth
    model = _student(dtype)
    depth = len(model.blocks)
    x = synth.video(2, 4, 64).cuda()
    outs = {}
    for on in (True, False):
        with _switch(on), torch.no_grad():
            outs[on], n = _counted(lambda: model(x))
        assert n == (depth if on else 0)
    a, b = _flat(outs[True]), _flat(outs[False])
    assert len(a) == len(b) == 8
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.isfinite(s.float()).all() and torch.equal(s, t), f"output {i} differs between the forward-only region and the training forward"
    # with gradients enabled the counter stays 0 whatever the switch says
    for on in (True, False):
        with _switch(on):
            out, n = _counted(lambda: model(x))
        assert n == 0 and out[2][0].requires_grad
    # training mode with stochastic depth, under no_grad: a block on its drop-path branch keeps the training forward.  (The rates are linspace(0, rate, depth):
    # block 0's is 0 and that block is on no training-only branch -- so every block is given the rate here.)
    model = _student(dtype, drop_path_rate=0.1).train()
    assert [blk.drop_path_rate for blk in model.blocks][0] == 0.0
    with _switch(True), torch.no_grad():
        _, n = _counted(lambda: model(x))
        assert n == 1                          # block 0 alone
        for blk in model.blocks:
            blk.drop_path_rate = 0.1
        _, n = _counted(lambda: model(x))
        assert n == 0


# ------------------------------------------------------------------------------------------------ 5. teacher
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_teacher_forward_is_bitwise_equal_with_the_switch_on_and_off(dtype):
    """99 tokens per clip, B = 3: 297 rows padded to 512"""
    from devias_amd import synth
    model = _teacher(dtype, 112)
    x = synth.video(3, 4, 112).cuda()
    outs = {}
    for on in (True, False):
        with _switch(on):
            outs[on], n = _counted(lambda: model(x))
        assert n == (len(model.blocks) if on else 0)
    for name, s, t in zip(("token", "logits"), outs[True], outs[False]):
        assert s.shape[0] == 3 and torch.isfinite(s.float()).all() and torch.equal(s, t), f"{name} differs"
    assert outs[True][1].float().abs().max() > 0


# ------------------------------------------------------------------------------------------------ 6. engine
def test_scene_test_file_and_merge_on_real_models(tmp_path):
    from devias_amd import synth
    from devias_amd.engine_for_slot import final_test_with_scene_label, merge
    model, teacher = _student("bf16"), _teacher("bf16", 64, num_classes=6)
    nb = model.num_classes
    loader = []
    for b in range(2):
        x = synth.video(3, 4, 64, first=3 * b)
        loader.append((x, torch.zeros(3, dtype=torch.long), ["clip%d" % (3 * b + i) for i in range(3)], torch.tensor([b, b + 1, b + 2]), torch.tensor([0, 1, 2])))
    path = tmp_path / "0.txt"
    stats = final_test_with_scene_label(loader, model, teacher, DEV, str(path), num_labels=nb)
    # the lines rebuilt from the models' own outputs
    lines, hit1, hit5, first = [], 0, 0, None
    with torch.no_grad():
        for x, _, ids, chunk, split in loader:
            out = model(x.cuda())[1][1].float()[:, nb:]
            tgt = teacher(x.cuda())[1].argmax(dim=1)
            top = out.topk(5, dim=1).indices
            h1, h5 = int((top[:, 0] == tgt).sum()), int((top == tgt[:, None]).any(dim=1).sum())
            hit1, hit5 = hit1 + h1, hit5 + h5
            first = "{}, {}\n".format(torch.tensor(h1, dtype=torch.float32) * 100. / 3, torch.tensor(h5, dtype=torch.float32) * 100. / 3)
            for i in range(3):
                lines.append("{} {} {} {} {}\n".format(ids[i], str(out[i].cpu().numpy().tolist()), int(tgt[i]), int(chunk[i]), int(split[i])))
    assert path.read_text() == first + "".join(lines)
    assert out.shape == (3, 6) and len(set(path.read_text().splitlines()[1:])) == 6
    assert stats["acc1"] == 100.0 * hit1 / 6 and stats["acc5"] == 100.0 * hit5 / 6
    top1, top5 = merge(str(tmp_path), 1)
    assert top1 == pytest.approx(100.0 * hit1 / 6, abs=1e-9) and top5 == pytest.approx(100.0 * hit5 / 6, abs=1e-9)
