"""Weight-only int8 decoding on the GPU: the row quantiser against its definition, the int8 skinny
GEMMs against fp64 on the dequantised weight with the bf16 skinny GEMMs as the yardstick (an error
of at most twice theirs, rows bit-independent of the row count), and the quantised captured step of
both decoder models against an fp64 model that holds the dequantised weights."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("N,K", [(40, 72), (16, 128), (1000, 128)])
def test_quantiser_bounds(N, K):
    from kubeml_amd.ops import decode as D
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.05).to(BF)
    w[N // 2] = 0
    q, scale = D.quant_rows_i8(w.to(dev))
    assert q.dtype == torch.int8 and q.shape == (N, K) and q.stride(0) % 16 == 0 and scale.shape == (N,)
    q, scale, wd = q.cpu(), scale.cpu(), w.double()
    want = (wd.abs().amax(1) / 127).float()
    ulp = lambda t: torch.nextafter(t.abs().float(), torch.tensor(float("inf"))) - t.abs().float()
    assert ((scale - want).abs() <= ulp(want)).all()
    assert int(q.abs().max()) <= 127 and int(q.abs().max()) == 127
    err = (wd - q.double() * scale.double()[:, None]).abs()
    assert (err <= scale.double()[:, None] / 2 + ulp(w).double()).all()
    assert scale[N // 2] == 0 and not q[N // 2].any()


@pytest.mark.parametrize("N,K,splits,act,bias", [
    (40, 72, None, None, False),            # N tail, K tail inside a chunk
    (48, 3072, None, None, False),          # split by the plan
    (128, 512, 4, None, False),             # forced split
    (32768, 64, None, None, False),         # the 4-wave shape
    (1536, 576, None, "gelu_tanh", True)])
def test_gemm_skinny_w8_against_fp64(N, K, splits, act, bias):
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(N * 7 + K)
    q, scale = D.quant_rows_i8((torch.randn(N, K, generator=g) * 0.1).to(BF).to(dev))
    x16, deq = torch.randn(16, K, generator=g).to(BF), q.double().cpu() * scale.double().cpu()[:, None]
    b = torch.randn(N, generator=torch.Generator().manual_seed(3)) if bias else None
    bg = None if b is None else b.to(dev)
    wy = deq.to(BF).to(dev)   # the yardstick's weight: the dequantised one rounded to bf16
    full = None
    for M in (16, 3, 1):
        xg = x16[:M].to(dev).contiguous()
        ref = x16[:M].double() @ deq.t()
        if b is not None:
            ref = ref + b.double()
        if act:
            ref = torch.nn.functional.gelu(ref, approximate="tanh")
        y = D.gemm_skinny_w8(xg, q, scale, bg, act=act, splits=splits)
        e, ey = _rel(y, ref), _rel(D.gemm_skinny(xg, wy, bg, act=act), ref)
        print(f"N {N} K {K} M {M}: int8 {e:.3e}, gemm_skinny on the rounded dequantised weight {ey:.3e}")
        assert y.shape == (M, N) and e <= 2.0 * ey
        if M == 16:
            full = y
        else:   # a row's result does not depend on M or on the other rows
            assert torch.equal(y, full[:M])
    for m in (5, 15):
        assert torch.equal(D.gemm_skinny_w8(x16[m:m + 1].to(dev).contiguous(), q, scale, bg, act=act, splits=splits),
                           full[m:m + 1])


@pytest.mark.parametrize("I,K,splits", [(352, 128, None), (344, 128, None), (128, 512, 4)])
def test_gemm_skinny_glu_w8_against_fp64(I, K, splits):
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import transformer as T
    g = torch.Generator().manual_seed(I * 7 + K)
    q, scale = D.quant_rows_i8((torch.randn(2 * I, K, generator=g) * 0.1).to(BF).to(dev))
    x16, deq = torch.randn(16, K, generator=g).to(BF), q.double().cpu() * scale.double().cpu()[:, None]
    wy = deq.to(BF).to(dev)
    full = None
    for M in (16, 3, 1):
        xg = x16[:M].to(dev).contiguous()
        gu = x16[:M].double() @ deq.t()
        ref = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        y = D.gemm_skinny_glu_w8(xg, q, scale, splits=splits)
        e, ey = _rel(y, ref), _rel(T.swiglu_fwd(D.gemm_skinny(xg, wy)), ref)
        print(f"I {I} K {K} M {M}: int8 fused {e:.3e}, gemm_skinny + swiglu_fwd {ey:.3e}")
        assert y.shape == (M, I) and e <= 2.0 * ey
        if M == 16:
            full = y
        else:
            assert torch.equal(y, full[:M])
    for m in (5, 15):
        assert torch.equal(D.gemm_skinny_glu_w8(x16[m:m + 1].to(dev).contiguous(), q, scale, splits=splits),
                           full[m:m + 1])


@pytest.mark.parametrize("family", ["llama", "gpt2"])
def test_quantised_step_against_fp64_and_undo(family):
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import Linear, flatten_module
    make = llama_tiny if family == "llama" else gpt2_tiny
    ref = make().double().eval()
    gpu = make(seed=1)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev).eval()
    flatten_module(gpu)
    with pytest.raises(ValueError):
        ref.quantize_decode_weights("int8")   # no int8 CPU path
    plens, steps = (37, 20), 8
    g = torch.Generator().manual_seed(5)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    ids = torch.randint(1, 1000, (2, L), generator=g) * mask
    forced = torch.randint(0, 1000, (2, steps), generator=g)
    caches = {d: ref.new_cache(2, L + steps, d) if d == "cpu" else gpu.new_cache(2, L + steps, d) for d in ("cpu", dev)}

    def run(pre, model, d):
        """the prompt through `pre` (bf16 / unquantised either way), then the forced steps through `model`"""
        with torch.no_grad():
            pre.prefill_logits(ids.to(d), mask.to(d), caches[d])
            return [model.decode_logits(caches[d], forced[:, t].to(d)).double().cpu() for t in range(steps)]

    plain = run(gpu, gpu, dev)
    e_bf16 = max(_rel(a, b) for a, b in zip(plain, run(ref, ref, "cpu")))
    names = list(gpu.state_dict())
    assert gpu.quantize_decode_weights("int8") == []
    assert list(gpu.state_dict()) == names
    refq = copy.deepcopy(ref)
    for (name, m), mq in zip(gpu.named_modules(), refq.modules()):
        if isinstance(m, Linear):
            assert m.w8.dtype == torch.int8, name
            deq = (m.w8.double() * m.w8_scale.double()[:, None]).cpu()[:m.out_features, :m.in_features]
            mq.weight = torch.nn.Parameter(deq)   # a parameter of its own: a tied token table keeps its values
    quant = run(gpu, gpu, dev)   # the same cache: its bf16 capture must not be replayed
    worst = max(_rel(a, b) for a, b in zip(quant, run(ref, refq, "cpu")))
    print(f"{family}: int8 decode steps vs fp64 on the dequantised weights {worst:.4f}, bf16 steps vs fp64 {e_bf16:.4f}")
    assert not torch.equal(quant[0], plain[0])
    assert worst <= 2.0 * e_bf16
    assert gpu.quantize_decode_weights(None) == [] and not any("w8" in n for n, _ in gpu.named_buffers())
    assert torch.equal(run(gpu, gpu, dev)[0], plain[0])
    out = gpu.generate(ids.to(dev), mask.to(dev), max_new_tokens=4)
    gpu.quantize_decode_weights("int8")
    assert gpu.generate(ids.to(dev), mask.to(dev), max_new_tokens=4).shape == out.shape
