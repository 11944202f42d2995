"""K5 on the GPU: ``ops.cu_sweep`` - a clean run over every CU at the full LDS size,
the smallest LDS sizes, partial coverage, a fault injected on one CU per sub-test
(a bit flipped in a value the kernel already computed; nothing faults), and the
wrapper's argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ITERS = 2
MAGIC = 0x4B355357
SUBTESTS = ("lds", "valu", "mfma_bf16", "mfma_fp8")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nvidia_terraform_modules_amd import ops as o
    return o


def keys_of(ops, rec):
    return np.array([ops.cu_sweep_decode(int(r["hw_id"]), int(r["xcc_id"]))["key"] for r in rec])


def assert_clean(rec):
    assert (rec["magic"] == MAGIC).all()
    assert not rec["bad"].any() and not rec["first"].any(), rec[rec["bad"].any(axis=1)][:4]
    assert (rec["wg"] == np.arange(len(rec))).all() and (rec["simd"] < 4).all()


@pytest.fixture(scope="module")
def clean_launch(ops):
    """One clean launch at the defaults (full LDS, 4 workgroups per CU): shared, never changed."""
    rec = ops.cu_sweep("cuda:0", iters=ITERS)
    rec.setflags(write=False)
    return rec


def test_clean_run_covers_every_cu_at_full_lds(ops, clean_launch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lds = ops.cu_sweep_max_lds_bytes("cuda:0")
    print(f"cus {cus} lds_bytes {lds}")
    assert lds >= 64 * 1024 and lds % 16 == 0
    recs, launches = [clean_launch], 1
    assert len(clean_launch) == 4 * cus
    while len(set(keys_of(ops, np.concatenate(recs)))) < cus and launches < 8:
        recs.append(ops.cu_sweep("cuda:0", iters=ITERS, seed=launches))
        launches += 1
    allrec = np.concatenate(recs)
    for r in recs:
        assert_clean(r)
    keys = set(keys_of(ops, allrec))
    s = ops.cu_sweep_summarize(allrec, cus, launches)
    print({k: s[k] for k in ("cus_covered", "simds_covered", "launches", "wg_per_cu_min", "wg_per_cu_max")})
    assert len(keys) == cus, (len(keys), cus, launches)      # a wrong decode splits or merges keys
    assert s["ok"] and s["cus_covered"] == cus and s["bad_cus"] == [] and s["message"] == ""
    assert s["simds_covered"] <= 4 * cus


def test_check_model_runs_the_coverage_loop(ops):
    from nvidia_terraform_modules_amd.models import cu_sweep_check
    s = cu_sweep_check(torch.device("cuda:0"), iters=ITERS)
    assert s["ok"] and s["cus_covered"] == s["cus"] and 1 <= s["launches"] <= 8, s
    assert s["lds_bytes"] == ops.cu_sweep_max_lds_bytes("cuda:0") and s["bad_cus"] == []


@pytest.mark.parametrize("lds_bytes", [16, 48])
def test_smallest_lds_sizes(ops, lds_bytes):
    # 16: one 16-byte access by one lane; 48: a ragged tail far below one access per wave
    rec = ops.cu_sweep("cuda:0", iters=1, lds_bytes=lds_bytes, grid=1)
    assert len(rec) == 1
    assert_clean(rec)


def test_partial_coverage_is_reported_not_marked_bad(ops):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rec = ops.cu_sweep("cuda:0", iters=ITERS, grid=8)
    assert_clean(rec)
    s = ops.cu_sweep_summarize(rec, cus)
    assert 1 <= s["cus_covered"] <= 8 and s["bad_cus"] == [] and s["workgroups"] == 8
    assert not s["ok"] and f"of {cus} CUs ran no workgroup after 1 launch" in s["message"]


@pytest.mark.parametrize("subtest", SUBTESTS)
def test_injected_fault_is_pinned_to_its_cu_and_subtest(ops, clean_launch, subtest):
    keys = sorted(set(keys_of(ops, clean_launch)))
    key = keys[len(keys) // 2]
    rec = ops.cu_sweep("cuda:0", iters=ITERS, fault_key=key, fault_subtest=subtest)
    assert (rec["magic"] == MAGIC).all()
    on_cu = keys_of(ops, rec) == key
    sub = SUBTESTS.index(subtest)
    bad = rec["bad"].any(axis=1)
    # the dispatcher need not place this launch's workgroups as the clean one's: what must hold
    # is that exactly the workgroups on the CU are bad (none, should none have run there)
    print(f"key {key:#x}: {int(on_cu.sum())} workgroup(s) on the CU")
    assert np.array_equal(bad, on_cu)
    assert on_cu.any(), "no workgroup ran on the chosen CU in this launch"
    for r in rec[on_cu]:
        assert r["bad"][sub] == 1 and r["bad"].sum() == 1, r
        assert int(r["first"]) & 0xFF == 1 + sub and r["first_round"] == 0
        x = int(r["expected"]) ^ int(r["got"])
        assert x and x & (x - 1) == 0, (hex(int(r["expected"])), hex(int(r["got"])))
    assert not rec["first"][~on_cu].any()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = ops.cu_sweep_summarize(rec, cus)
    assert [b["key"] for b in s["bad_cus"]] == [key] and s["bad_cus"][0]["subtests"] == [subtest]
    assert s["bad_cus"][0]["bad_workgroups"] == s["bad_cus"][0]["workgroups"] == int(on_cu.sum())


def test_argument_refusals_launch_nothing(ops, monkeypatch):
    from nvidia_terraform_modules_amd.ops.gpu import cu_sweep as kernels

    class NoLaunch:
        def __getattr__(self, name):
            if name == "ntm_cu_sweep_launch":
                raise AssertionError("a refused call reached the launch")
            return getattr(real, name)

    real = kernels.lib()
    monkeypatch.setattr(kernels, "lib", lambda: NoLaunch())
    limit = ops.cu_sweep_max_lds_bytes("cuda:0")
    for bad in (24, 0, limit + 16):
        with pytest.raises(ValueError):
            ops.cu_sweep("cuda:0", iters=1, lds_bytes=bad, grid=1)
    with pytest.raises(ValueError):
        ops.cu_sweep("cuda:0", iters=1, grid=1, fault_key=0)          # no sub-test named
    with pytest.raises(ValueError):
        ops.cu_sweep("cuda:0", iters=1, grid=1, fault_key=0, fault_subtest="sfu")
