"""K14 on the GPU: ``ops.gpu.pda.pda_fwd`` (ntm_pda_fwd: the split kernel and the combine) bitwise
against K13's reference kernel on the gathered keys of exact inputs, within the derived tolerance
on dense ones, and its edges: empty splits and waves, a one-key sequence, rows that see no key in
a split, NaN page tails and a NaN poison page, prefix-shared pages, canaries round every output and
the workspace, determinism, the CU table, the argument contract, ``pda_check``."""
import re

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd.models.checks.pda import pda_check
from nvidia_terraform_modules_amd.ops import attn as A
from nvidia_terraform_modules_amd.ops import pda as P
from nvidia_terraform_modules_amd.ops.gpu import attn as GA
from nvidia_terraform_modules_amd.ops.gpu import pda as G

pytestmark = pytest.mark.gpu

# (Hq, Hkv, T, lens, S, prefix-shared pairs)
EXACT = [(8, 2, 1, [257, 1], 4, 0),      # empty splits and waves; a one-key last page
         (4, 1, 4, [191], 1, 0),         # causal among the new tokens; the single-split path
         (32, 1, 1, [300], 2, 0),        # all 32 rows
         (2, 2, 1, [64, 1000], 3, 1),    # G = 1; uneven splits; sequence 1 reads sequence 0's first pages
         (32, 8, 4, [5, 130], 2, 0),     # a row that sees 2 keys; rows with no key in a split
         (16, 2, 1, [2048], 8, 0)]       # wave strides


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


def _args(d):
    return d["q"], d["k_pool"], d["v_pool"], d["block_table"], d["seq_lens"]


@pytest.fixture(scope="module")
def exact_257(dev):
    """One exact problem and its reference, shared by the tests that do not need their own."""
    pr = P.pda_make_problem("exact", 8, 2, 1, [257, 1], seed=0x14 + 258)
    d = G.pda_to_device(pr, dev)
    return pr, d, G.pda_reference_gpu(*_args(d), scale_log2=1.0)


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s[:3])) + "_" + "_".join(map(str, s[3])) + "_S" + str(s[4]))
def test_exact_inputs_are_bitwise_on_o_m_and_l(dev, shape):
    Hq, Hkv, T, lens, S, shared = shape
    pr = P.pda_make_problem("exact", Hq, Hkv, T, lens, seed=0x14 + sum(lens), shared_pairs=shared)
    for s in pr["seqs"]:
        assert A.attn_exact(s["qi"], s["ki"], s["vi"], True)
    assert (pr["k_pool"][pr["pt"]["poison"]] == 0x7FC0).all() and (pr["v_pool"][pr["pt"]["poison"]] == 0x7FC0).all()
    tail = lens[-1] % 16                                       # NaN page tail past len, where the last page is ragged
    if tail:
        assert (pr["k_pool"][pr["block_table"][-1, (lens[-1] - 1) // 16], :, tail:] == 0x7FC0).all()
    if shared:
        assert (pr["block_table"][1, :2] == pr["block_table"][0, :2]).all()
    d = G.pda_to_device(pr, dev)
    o, m, l = G.pda_fwd(*_args(d), splits=S, scale_log2=1.0, return_stats=True)
    ref = G.pda_reference_gpu(*_args(d), scale_log2=1.0)
    host = P.pda_reference_f32(pr)  # the reference kernel on gathered keys against its numpy twin
    assert not _first(_bits(ref["o"]), host["o"]) and not _first(_bits(ref["l"]), host["l"].view(np.uint32))
    assert not _first(_bits(m), _bits(ref["m"])), "m"
    assert not _first(_bits(l), _bits(ref["l"])), "l"
    assert not _first(_bits(o), _bits(ref["o"])), "O"
    for e, g in ((ref["o"], o), (ref["m"], m), (ref["l"], l)):
        assert GA.attn_compare(e, g).ok
    assert not torch.isnan(o.float()).any() and (host["o"] != 0).mean() > 0.5


def test_dense_inputs_are_within_the_derived_tolerance(dev):
    Hq, Hkv, T, lens, S = 8, 2, 1, [320, 77, 513], 3
    pr = P.pda_make_problem("dense", Hq, Hkv, T, lens, seed=3)
    d = G.pda_to_device(pr, dev)
    o = G.pda_fwd(*_args(d), splits=S)
    ref = G.pda_reference_gpu(*_args(d))
    err = (o.float() - ref["o32"]).abs().double()
    a = ref["a"].double()
    print("dense worst err / a", float((err / a.clamp_min(1e-30)).max()))
    assert bool((err <= 2.0 ** -7 * a + 2.0 ** -20).all())
    # and the default scale is 1 / sqrt(128): torch's fp32 softmax on the gathered keys agrees to bf16 accuracy
    for b, n in enumerate(lens):
        k = G.pda_gather(d["k_pool"], d["block_table"], d["seq_lens"], b).float().repeat_interleave(Hq // Hkv, 1)
        v = G.pda_gather(d["v_pool"], d["block_table"], d["seq_lens"], b).float().repeat_interleave(Hq // Hkv, 1)
        want = torch.softmax(d["q"][b:b + 1].float() @ k.transpose(2, 3) / 128 ** 0.5, dim=-1) @ v
        assert float((o[b:b + 1].float() - want).abs().max()) < 2e-2


def test_one_split_and_four_splits_give_equal_bits(dev, exact_257):
    pr, d, ref = exact_257
    one = G.pda_fwd(*_args(d), splits=1, scale_log2=1.0, return_stats=True)
    four = G.pda_fwd(*_args(d), splits=4, scale_log2=1.0, return_stats=True)
    for x, y, want in zip(one, four, (ref["o"], ref["m"], ref["l"])):
        assert not _first(_bits(x), _bits(y)) and not _first(_bits(x), _bits(want))


def test_two_launches_give_equal_bits(dev):
    d = G.pda_to_device(P.pda_make_problem("dense", 8, 2, 1, [320, 77, 513], seed=9), dev)
    a = G.pda_fwd(*_args(d), splits=3, return_stats=True)
    b = G.pda_fwd(*_args(d), splits=3, return_stats=True)
    for x, y in zip(a, b):
        assert not _first(_bits(x), _bits(y))


def test_canaries_round_every_output_and_the_workspace_stay_untouched(dev, exact_257):
    pr, d, ref = exact_257
    B, Hq, Hkv, T, S = 2, 8, 2, 1, 4
    rows, ws = B * Hq * T, P.pda_workspace_bytes(B, Hkv, S) // 4
    obuf = torch.full(((rows + 2) * 128,), -7.0, dtype=torch.bfloat16, device=dev)
    mbuf = torch.full((rows + 256,), -7.0, dtype=torch.float32, device=dev)
    lbuf = torch.full((rows + 256,), -7.0, dtype=torch.float32, device=dev)
    wbuf = torch.full((ws + 256,), -7.0, dtype=torch.float32, device=dev)
    out = (obuf[128:128 + rows * 128], mbuf[128:128 + rows], lbuf[128:128 + rows], wbuf[128:128 + ws])
    G.pda_fwd(*_args(d), splits=S, scale_log2=1.0, out=out)
    for buf, n, want in ((obuf, rows * 128, ref["o"]), (mbuf, rows, ref["m"]), (lbuf, rows, ref["l"]), (wbuf, ws, None)):
        assert bool((buf[:128] == -7.0).all()) and bool((buf[128 + n:] == -7.0).all())
        if want is not None:
            assert torch.equal(buf[128:128 + n].view(want.shape), want)
    # every workspace word was written: (b, hkv, s) partials of acc [32][128], m[32], l[32], empty splits included
    assert not bool((wbuf[128:128 + ws] == -7.0).all()) and P.pda_split_range(1, 3, 4) == (1, 1)
    part = wbuf[128:128 + ws].view(B * Hkv * S, P.PDA_PARTIAL_FLOATS)
    empty = part[(1 * Hkv + 0) * S + 3]                        # sequence 1 (one key), split 3: no step at all
    assert bool((empty[:4096] == 0).all()) and bool(torch.isneginf(empty[4096:4128]).all()) and bool((empty[4128:] == 0).all())


def test_cu_table_shows_more_than_one_xcd(dev, exact_257):
    pr, d, ref = exact_257
    o, table = G.pda_fwd(*_args(d), splits=4, scale_log2=1.0, table=True)
    t = table.cpu().numpy().view(np.uint32)
    assert t.shape == (P.pda_grid(2, 2, 4), 2)
    xcds = {A.attn_decode_cu(int(hw), int(xcc))[0] for hw, xcc in t}
    assert len(xcds) > 1, xcds


def test_argument_contract(dev, exact_257):
    pr, d, ref = exact_257
    q, kp, vp, bt, sl = _args(d)
    bf = dict(dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="G \\* T"):                           # G * T > 32
        G.pda_fwd(torch.zeros((2, 66, 1, 128), **bf), kp, vp, bt, sl)
    with pytest.raises(ValueError, match="G \\* T"):
        G.pda_fwd(torch.zeros((2, 32, 4, 128), **bf), kp, vp, bt, sl)
    with pytest.raises(ValueError, match="T <= len"):                          # len < T: sequence 1 holds one key
        G.pda_fwd(torch.zeros((2, 8, 2, 128), **bf), kp, vp, bt, sl)
    flat = torch.zeros((kp.numel() + 8,), **bf)
    with pytest.raises(ValueError, match="16-byte aligned"):                   # a pool that is not 16-byte aligned
        G.pda_fwd(q, flat[4:4 + kp.numel()].view(kp.shape), vp, bt, sl)
    with pytest.raises(ValueError, match="int32"):                             # a block table of the wrong dtype
        G.pda_fwd(q, kp, vp, bt.long(), sl)
    with pytest.raises(ValueError, match="head dimension must be 128"):        # a head dimension of 64
        G.pda_fwd(torch.zeros((2, 8, 1, 64), **bf), kp, vp, bt, sl)
    with pytest.raises(ValueError, match="page id"):                           # an id outside the pool is refused, not read
        G.pda_fwd(q, kp, vp, torch.full_like(bt, kp.shape[0]), sl)
    with pytest.raises(ValueError, match="splits"):
        G.pda_fwd(q, kp, vp, bt, sl, splits=65)
    with pytest.raises(ValueError, match="needs m and l"):
        G.pda_fwd(q, kp, vp, bt, sl, return_stats=True, out=(torch.empty_like(q), None, None))
    assert G.pda_fwd(q, kp, vp, bt, sl, scale_log2=1.0).shape == q.shape       # the default S
    from nvidia_terraform_modules_amd.ops._lib import lib
    assert lib().ntm_pda_lds_bytes() == P.PDA_LDS_BYTES
    assert lib().ntm_pda_default_splits(32, 8, 8192, 256) == P.pda_splits(32, 8, 8192, 256) == 2
    assert lib().ntm_pda_workspace_bytes(2, 8, 3) == P.pda_workspace_bytes(2, 8, 3)


def test_pda_check_on_the_gpu_and_its_injection(dev):
    r = pda_check(dev)
    print({k: v for k, v in r.items() if k != "message"})
    assert r["ok"] and r["xcds"] > 1 and 0 < r["dense_worst"] < 2.0 ** -7, r
    bad = pda_check(dev, corrupt=True)
    assert not bad["ok"] and len(bad["failures"]) == 1 and bad["bad"]["exact"] == 1, bad
    line = bad["failures"][0]
    assert re.match(r"gpu0: pda exact T1 O: seq \d+ head \d+ tok 0 col \d+: cu( \d+\.\d+\.\d+\.\d+){4} \(xcd\.se\.sh\.cu\): expected "
                    r"0x[0-9a-f]{8}, got 0x[0-9a-f]{8}, bad bits 0x00080000; 1 differ$", line) and len(line) < 200, line
