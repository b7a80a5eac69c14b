"""devias_wgrad_group (csrc/gemm_wgrad_group.hip): several weight gradients dW_j [Nout_j, Kin_j] (fp32) = beta dW_j + dY_j^T X_j over the same M rows as ONE grouped
split-K launch + one combine.  Small shapes reach every schedule form through `cus_override`: rounds without a split (the unit writes dW, beta honoured), split rounds
(partial tiles + the combine), rounds that do not fill the workgroups, more than one round, ragged last slabs (17 K-tiles).  Every element is held to the
weight-gradient bound of tests/kernel_bounds.py against float64 on graded inputs; two runs are bitwise equal; the launch counters say one gemm256 per job; and a job
whose plan is ONE uniform round is bitwise devias_gemm's split-K product (same slabs, same kernel arithmetic, same reduce order)."""
import pytest
import torch

import embedded_operands as eo
import kernel_bounds as kb
from devias_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
JOBS = [(256, 256), (512, 256), (256, 768)]          # (Nout, Kin)
_CACHE = {}


def operands(M, njobs=3):
    """graded operands, their float64 products and bound parts, once per M (shared, never modified)"""
    if (M, njobs) not in _CACHE:
        out = []
        for j in range(njobs):
            N, K = JOBS[j % 3]
            dY = (kb._randn((M, N), 701 + 10 * j, DEV) * kb.graded(N, 6, DEV).float()[None, :] * kb.graded(M, 3, DEV).float()[:, None]).to(BF)
            X = (kb._randn((M, K), 702 + 10 * j, DEV) * kb.graded(K, 6, DEV).float()[None, :]).to(BF)
            c_old = kb._randn((N, K), 703 + 10 * j, DEV) * kb.graded(N, 6, DEV).float()[:, None] * kb.graded(K, 6, DEV).float()[None, :] * 8.0
            refs = {beta: kb.gemm_ref(dY.t(), X, BF, out_f32=True, beta=beta, c_old=c_old)["out"] for beta in (0.0, 1.0)}
            out.append((dY, X, c_old, refs))
        _CACHE[(M, njobs)] = out
    return _CACHE[(M, njobs)]


def run(ops_, M, cus, beta, njobs=3):
    data = operands(M, njobs)
    outs = [c_old.clone() for _, _, c_old, _ in data]
    ops_.wgrad_group([ops_.wgrad_job(dY, X, o, beta) for (dY, X, _, _), o in zip(data, outs)], cus=cus)
    torch.cuda.synchronize()
    return outs


def forms(rounds, cus):
    return {"unsplit": any(s == 1 for _, s in rounds), "split": any(s > 1 for _, s in rounds), "unfilled": any(t * s < cus for t, s in rounds), "rounds": len(rounds)}


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("cus", [8, 16])
@pytest.mark.parametrize("M", [512, 1088])
def test_three_jobs_one_call(M, cus, beta):
    tiles = [(n // 256) * (k // 256) for n, k in JOBS]
    rounds, _ = ops.wgrad_group_plan(tiles, M // 64, cus)
    ops.counters(reset=True)
    outs = run(ops, M, cus, beta)
    cnt = ops.counters()
    again = run(ops, M, cus, beta)
    split = any(s > 1 for _, s in rounds)
    assert cnt["gemm256"] == 3 and cnt["splitk_reduce"] == int(split) and cnt["gemm128_bf16"] == 0, (cnt, rounds)
    for j, ((dY, X, c_old, refs), out, out2) in enumerate(zip(operands(M), outs, again)):
        ref, bound = refs[beta]
        r = kb.check(f"job {j} {JOBS[j]} M {M} cus {cus} beta {beta} plan {rounds}", out, ref, bound, lambda i, K=JOBS[j][1]: kb.where2d(i, K))
        print(f"wgrad_group M={M} cus={cus} beta={beta} job {j}: plan {rounds} worst |out - ref| / bound = {r:.3g}")
        assert torch.equal(out, out2), f"job {j}: two runs differ"


def test_schedule_forms_all_occur():
    """over the cases above: rounds without a split, split rounds, rounds that leave workgroups idle; and (below) a plan of more than one round"""
    seen = {"unsplit": False, "split": False, "unfilled": False}
    tiles = [(n // 256) * (k // 256) for n, k in JOBS]
    for M in (512, 1088):
        for cus in (8, 16):
            f = forms(ops.wgrad_group_plan(tiles, M // 64, cus)[0], cus)
            for k in seen:
                seen[k] = seen[k] or f[k]
    assert all(seen.values()), seen


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_more_than_one_round(beta):
    """six jobs (12 tiles) on 8 workgroups, 17 K-tiles: several rounds, split and unsplit, in one launch"""
    M, cus = 1088, 8
    tiles = [(n // 256) * (k // 256) for n, k in JOBS] * 2
    rounds, _ = ops.wgrad_group_plan(tiles, M // 64, cus)
    assert len(rounds) > 1, rounds
    ops.counters(reset=True)
    outs = run(ops, M, cus, beta, njobs=6)
    assert ops.counters()["gemm256"] == 6
    again = run(ops, M, cus, beta, njobs=6)
    for j, ((dY, X, c_old, refs), out, out2) in enumerate(zip(operands(M, 6), outs, again)):
        ref, bound = refs[beta]
        r = kb.check(f"job {j} plan {rounds} beta {beta}", out, ref, bound, lambda i, K=JOBS[j % 3][1]: kb.where2d(i, K))
        print(f"wgrad_group six jobs beta={beta} job {j}: plan {rounds} worst ratio {r:.3g}")
        assert torch.equal(out, out2)


@pytest.mark.parametrize("M", [512, 1088])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_one_uniform_round_is_bitwise_the_split_k_gemm(M, beta):
    """one job of T = 2 tiles, split s = 4 on T * s = 8 workgroups: the same slabs (devias_gemm's rule), the same K loop and epilogue, the same reduce order"""
    N, K, s = 512, 256, 4
    rounds, _ = ops.wgrad_group_plan([2], M // 64, 2 * s)
    assert rounds == [(2, s)], rounds
    dY, X, c_old, _ = operands(M)[1]
    assert (dY.shape[1], X.shape[1]) == (N, K)
    want = c_old.clone()
    ops.gemm(dY, X, trans_a=True, trans_b=True, out_f32=True, split_k=s, out=want, beta=beta)
    got = c_old.clone()
    ops.wgrad_group([ops.wgrad_job(dY, X, got, beta)], cus=2 * s)
    torch.cuda.synchronize()
    assert torch.equal(got, want), float((got - want).abs().max())


def test_ineligible_lists_are_refused():
    dY, X, c_old, _ = operands(512)[0]
    out = c_old.clone()
    with pytest.raises(ValueError):            # different M in one call
        ops.wgrad_group([ops.wgrad_job(dY, X, out), ops.wgrad_job(dY[:256], X[:256], out)], cus=8)
    with pytest.raises(ValueError):            # not whole 256 x 256 tiles
        ops.wgrad_group([ops.wgrad_job(dY[:, :128].contiguous(), X, out[:128])], cus=8)
    with pytest.raises(ValueError):            # M not a multiple of the K-tile
        ops.wgrad_group([ops.wgrad_job(dY[:96], X[:96], out)], cus=8)
    torch.cuda.synchronize()
    assert torch.equal(out, c_old)


# ---- embedded operands (tests/embedded_operands.py): ldy > Nout, ldx > Kin, NaN between and behind the rows of dY and X, dW and the workspace inside canary bands ----
def _group_call(jobs, cus, ws_tail=0):
    """devias_wgrad_group with a workspace of exactly the queried size followed by `ws_tail` canary floats; returns the workspace buffer and its used length"""
    from devias_amd import _lib
    lib = _lib.load()
    arr = (_lib.WgradJob * len(jobs))(*jobs)
    nbytes = lib.devias_wgrad_group_workspace_bytes(arr, len(jobs), cus)
    assert nbytes >= 0, lib.devias_last_error()
    ws = torch.full((nbytes // 4 + ws_tail,), eo.CANARY, device=DEV)
    _lib.check(lib.devias_wgrad_group(arr, len(jobs), cus, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "devias_wgrad_group")
    torch.cuda.synchronize()
    return ws, nbytes // 4


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("cus", [8, 16])
def test_three_jobs_embedded_operands(cus, beta):
    """the three jobs of test_three_jobs_one_call at M = 512 (cus 8: a split round; 16: another plan) with dY and X at leading dimensions Nout + 8 (j + 1) and
    Kin + 8 (j + 2): bitwise the dense call's dW, nothing written outside dW or past the workspace's queried size, inputs untouched"""
    M = 512
    data = operands(M)
    dense = run(ops, M, cus, beta)
    jobs, bands, inputs = [], [], []
    for j, (dY, X, c_old, _) in enumerate(data):
        ybuf, yv = eo.embed(dY, dY.shape[1] + 8 * (j + 1), 64, eo.TAIL_ROWS, eo.NAN)
        xbuf, xv = eo.embed(X, X.shape[1] + 8 * (j + 2), 64, eo.TAIL_ROWS, eo.NAN)
        src = c_old if beta != 0.0 else torch.full_like(c_old, eo.NAN)              # beta = 0: a dW the call must not read
        wbuf, wv = eo.embed(src, c_old.shape[1], 64, eo.TAIL_ROWS, eo.CANARY)
        jobs.append(eo.wgrad_job_raw(yv, xv, wv, beta))
        assert (jobs[-1].ldy, jobs[-1].ldx) == (dY.shape[1] + 8 * (j + 1), X.shape[1] + 8 * (j + 2))
        bands.append((wbuf, wv)); inputs += [(ybuf, ybuf.clone()), (xbuf, xbuf.clone())]
    ops.counters(reset=True)
    ws, used = _group_call(jobs, cus, ws_tail=65536)
    assert ops.counters()["gemm256"] == 3
    assert bool((ws[used:] == eo.CANARY).all()), "a store past the queried workspace size"
    for j, ((wbuf, wv), want) in enumerate(zip(bands, dense)):
        assert eo.same_bits(wv, want), f"job {j}: dW differs from the dense call's"
        assert eo.intact(wbuf, tuple(wv.shape), wv.shape[1], 64, eo.CANARY), f"job {j}: a store outside dW"
    for buf, before in inputs:
        assert eo.same_bits(buf, before)


def test_bad_leading_dimensions_are_refused():
    """ldy % 8 != 0, ldy < Nout, ldx < Kin: DEVIAS_EINVAL from the size query and from the call, no counter moved, dW untouched"""
    from devias_amd import _lib
    lib = _lib.load()
    dY, X, c_old, _ = operands(512)[0]
    out = c_old.clone()
    ws = torch.empty(1 << 20, device=DEV)
    for field, value in (("ldy", dY.shape[1] + 4), ("ldy", dY.shape[1] - 8), ("ldx", X.shape[1] - 8)):
        job = eo.wgrad_job_raw(dY, X, out)
        setattr(job, field, value)
        arr = (_lib.WgradJob * 1)(job)
        before = ops.counters()
        assert lib.devias_wgrad_group_workspace_bytes(arr, 1, 8) == -1
        assert lib.devias_wgrad_group(arr, 1, 8, ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream) == -1        # DEVIAS_EINVAL
        assert f"{field}={value}" in lib.devias_last_error().decode()
        assert ops.counters() == before
    torch.cuda.synchronize()
    assert torch.equal(out, c_old)
