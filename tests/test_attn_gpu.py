"""K13 on the GPU: ``ops.gpu.attn.attn_fwd`` (ntm_attn_fwd) bitwise against the reference kernel on
exact inputs, within the derived tolerance on dense ones, and its edges: canaries round every
output, determinism, the CU table, the argument contract, ``attn_check``."""
import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd.models.checks.attn import attn_check
from nvidia_terraform_modules_amd.ops import attn as A
from nvidia_terraform_modules_amd.ops.gpu import attn as G

pytestmark = pytest.mark.gpu

# (B, Hq, Hkv, Sq, Sk, causal)
EXACT = [(1, 2, 1, 192, 192, False), (1, 2, 1, 192, 192, True), (1, 4, 2, 129, 191, False), (1, 4, 2, 129, 191, True),
         (2, 2, 2, 1, 257, True), (1, 1, 1, 128, 64, False)]
DENSE = [(2, 4, 2, 320, 320, False), (2, 4, 2, 320, 320, True), (1, 8, 2, 1024, 1024, False), (1, 8, 2, 1024, 1024, True)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(t: torch.Tensor) -> np.ndarray:
    raw = t.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)
    return raw.view(np.uint16 if t.element_size() == 2 else np.uint32).reshape(t.shape)


def _first(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    return "" if not len(bad) else f"{len(bad)} differ, first at {tuple(bad[0])}: expected {int(want[tuple(bad[0])]):#x}, got {int(got[tuple(bad[0])]):#x}"


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_exact_inputs_are_bitwise_on_o_m_and_l(dev, shape):
    B, Hq, Hkv, Sq, Sk, causal = shape
    i = A.attn_make_inputs("exact", B, Hq, Hkv, Sq, Sk, seed=0x4B3D + Sq)
    assert A.attn_exact(i["qi"], i["ki"], i["vi"], causal)
    d = G.attn_to_device(i, dev)
    o, m, l = G.attn_fwd(d["q"], d["k"], d["v"], causal=causal, scale_log2=1.0, return_stats=True)
    ref = G.attn_reference_gpu(d["q"], d["k"], d["v"], causal=causal, scale_log2=1.0)
    host = A.attn_reference_f32(i, causal)  # the reference kernel itself against its numpy twin
    assert not _first(_bits(ref["o"]), host["o"]) and not _first(_bits(ref["l"]), host["l"].view(np.uint32))
    assert not _first(_bits(m), _bits(ref["m"])), "m"
    assert not _first(_bits(l), _bits(ref["l"])), "l"
    assert not _first(_bits(o), _bits(ref["o"])), "O"
    for e, g in ((ref["o"], o), (ref["m"], m), (ref["l"], l)):
        assert G.attn_compare(e, g).ok
    assert (host["o"] != 0).mean() > 0.5


@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "x".join(map(str, s)))
def test_dense_inputs_are_within_the_derived_tolerance(dev, shape):
    B, Hq, Hkv, Sq, Sk, causal = shape
    d = G.attn_to_device(A.attn_make_inputs("dense", B, Hq, Hkv, Sq, Sk, seed=Sq), dev)
    o = G.attn_fwd(d["q"], d["k"], d["v"], causal=causal)
    ref = G.attn_reference_gpu(d["q"], d["k"], d["v"], causal=causal)
    err = (o.float() - ref["o32"]).abs().double()
    a = ref["a"].double()
    print(shape, "worst err / a", float((err / a.clamp_min(1e-30)).max()))
    assert bool((err <= 2.0 ** -7 * a + 2.0 ** -20).all())
    # and the default scale is 1 / sqrt(128): softmax(q k^T / sqrt(128)) v in fp32 agrees to bf16 accuracy
    rep = Hq // Hkv
    s = d["q"].float() @ d["k"].float().repeat_interleave(rep, 1).transpose(2, 3) / 128 ** 0.5
    s = s.masked_fill(~torch.from_numpy(A._visible(Sq, Sk, causal)).to(dev), float("-inf"))
    want = torch.softmax(s, dim=-1) @ d["v"].float().repeat_interleave(rep, 1)
    assert float((o.float() - want).abs().max()) < 2e-2


def test_canaries_round_every_output_stay_untouched(dev):
    B, Hq, Hkv, Sq, Sk = 1, 4, 2, 129, 191
    d = G.attn_to_device(A.attn_make_inputs("exact", B, Hq, Hkv, Sq, Sk, seed=2), dev)
    rows = B * Hq * Sq
    # one sentinel row before and a sentinel tail after each output (O rows are 256 bytes: 16-byte aligned)
    obuf = torch.full(((rows + 2) * 128,), -7.0, dtype=torch.bfloat16, device=dev)
    mbuf = torch.full((rows + 256,), -7.0, dtype=torch.float32, device=dev)
    lbuf = torch.full((rows + 256,), -7.0, dtype=torch.float32, device=dev)
    out = (obuf[128:128 + rows * 128], mbuf[128:128 + rows], lbuf[128:128 + rows])
    G.attn_fwd(d["q"], d["k"], d["v"], causal=True, scale_log2=1.0, out=out)
    ref = G.attn_reference_gpu(d["q"], d["k"], d["v"], causal=True, scale_log2=1.0)
    for buf, head, n, want in ((obuf, 128, rows * 128, ref["o"]), (mbuf, 128, rows, ref["m"]), (lbuf, 128, rows, ref["l"])):
        assert bool((buf[:head] == -7.0).all()) and bool((buf[head + n:] == -7.0).all())
        assert torch.equal(buf[head:head + n].view(want.shape), want)


def test_two_launches_give_equal_bits(dev):
    d = G.attn_to_device(A.attn_make_inputs("dense", 2, 4, 2, 320, 320, seed=9), dev)
    a = G.attn_fwd(d["q"], d["k"], d["v"], causal=True, return_stats=True)
    b = G.attn_fwd(d["q"], d["k"], d["v"], causal=True, return_stats=True)
    for x, y in zip(a, b):
        assert not _first(_bits(x), _bits(y))


def test_cu_table_shows_more_than_one_xcd(dev):
    d = G.attn_to_device(A.attn_make_inputs("exact", 2, 4, 2, 320, 320, seed=1), dev)
    o, table = G.attn_fwd(d["q"], d["k"], d["v"], scale_log2=1.0, table=True)
    t = table.cpu().numpy().view(np.uint32)
    assert t.shape == (A.attn_grid(2, 4, 320), 2)
    xcds = {A.attn_decode_cu(int(hw), int(xcc))[0] for hw, xcc in t}
    assert len(xcds) > 1, xcds


def test_argument_contract(dev):
    q = torch.zeros((1, 2, 64, 128), dtype=torch.bfloat16, device=dev)
    kv = torch.zeros((1, 1, 32, 128), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="causal needs Sk >= Sq"):
        G.attn_fwd(q, kv, kv, causal=True)
    q64 = torch.zeros((1, 2, 64, 64), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="head dimension must be 128"):
        G.attn_fwd(q64, q64, q64)
    with pytest.raises(ValueError):
        G.attn_fwd(torch.zeros((1, 3, 64, 128), dtype=torch.bfloat16, device=dev), torch.zeros((1, 2, 64, 128), dtype=torch.bfloat16, device=dev),
                   torch.zeros((1, 2, 64, 128), dtype=torch.bfloat16, device=dev))
    with pytest.raises(ValueError):
        G.attn_fwd(q.float(), kv, kv)
    assert G.attn_fwd(q, kv, kv).shape == q.shape  # non-causal with Sk < Sq is fine
    with pytest.raises(ValueError, match="O must be"):
        G.attn_fwd(q, kv, kv, out=(torch.empty((1, 64, 2, 128), dtype=torch.bfloat16, device=dev), None, None))
    with pytest.raises(ValueError, match="needs m and l"):
        G.attn_fwd(q, kv, kv, return_stats=True, out=(torch.empty_like(q), None, None))
    from nvidia_terraform_modules_amd.ops._lib import lib
    assert lib().ntm_attn_lds_bytes() == A.ATTN_LDS_BYTES


def test_attn_check_on_the_gpu_and_its_injection(dev):
    r = attn_check(dev)
    print({k: v for k, v in r.items() if k != "message"})
    assert r["ok"] and r["xcds"] > 1 and 0 < r["dense_worst"] < 2.0 ** -7, r
    bad = attn_check(dev, corrupt=True)
    assert not bad["ok"] and len(bad["failures"]) == 1 and " cu " in bad["failures"][0] and "bad bits 0x00080000" in bad["failures"][0]
