"""rlt_gemm_plan at K = 768 (no GPU: the plan is host code).  The attention in-projection's dX product, T x 256 x 768 accumulated in
place, was measured faster on gemm6e than on gemm6c once gemm6e's accumulate epilogue read C in batches, and so were the plain and
bias forms of that length, with B in either layout; csrc/gemm_plan.hip sends exactly that length there.  The lengths around it, which
no product of the models has, stay on gemm6c, and the epilogues gemm6e does not have stay there at K = 768 as well."""
import pytest

ACC, RELU, BF16X6 = 2, 1, 2
T = 4096 * 300


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def family(native, tb, M, K, flags=0, present=()):
    rc, plan = native.gemm_plan(native.gemm_call(0, tb, M, 256, K, flags=flags, present=present), BF16X6)
    assert rc == 0
    return plan["family"], plan["persistent"]


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("M,persistent", [(256, 0), (T, 1)])
def test_k768_runs_on_gemm6e(native, M, persistent, tb):
    for flags, present in ((0, ()), (0, ("bias",)), (ACC, ()), (ACC | RELU, ("bias",))):
        assert family(native, tb, M, 768, flags, present) == ("gemm6e", persistent), (flags, present)


@pytest.mark.parametrize("tb", [0, 1])
def test_the_lengths_around_it_and_the_mask_epilogues_stay_on_gemm6c(native, tb):
    for K in (512, 736, 800, 992):
        assert family(native, tb, T, K, ACC) == ("gemm6c", 1), K
    assert family(native, tb, T, 768, 0, ("relu_mask",)) == ("gemm6c", 1)
    assert family(native, tb, T, 768, 0, ("bits_in",)) == ("gemm6c", 1)
    assert family(native, tb, T, 1024, ACC) == ("gemm6e", 1)
