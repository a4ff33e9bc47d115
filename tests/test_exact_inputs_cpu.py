"""tests/exact_inputs.py can detect what it claims to detect (no GPU): for every case tests/test_exact_products_gpu.py runs, the operands are
exactly summable in fp32 (sum of absolute terms < 2^24 units of their grid); where an output sums at least 256 products, at least 10% of the
right answers are no bf16 number and at least 2% are ties that nearest-even rounds downward (conditions on the fixtures: a case that misses
one gets another seed or grid, not another floor); and every mutated reference -- one tap dropped, truncation, round-half-away, conv + bias
rounded before the residual, the bias through bf16 -- differs from the right answer in at least one element.  On one 64 -> 64 3x3 case the
single-tap and the truncation mutant pass the criterion the suite had (2^-7 * max(1, |ref|.max())) and fail assert_bits: the gap closed."""
import pytest
import torch

from tests import exact_inputs as X

CASES = [pytest.param(ops, refs, case, id=f"{name}-{case}") for name, cases, ops, refs in X.FAMILIES for case in cases]
MIN_PRODUCTS, MIN_INEXACT, MIN_TIES_DOWN = 256, 0.10, 0.02
ROUNDING_MUTANTS = ("truncation", "round-half-away", "rounded before the residual")        # what the floors are there to expose


@pytest.mark.parametrize("operands, refs, case", CASES)
def test_case_is_exactly_summable_sensitive_and_rejects_every_mutant(operands, refs, case):
    for label, ref in refs(operands(case)).items():
        what = f"{case} {label}"
        units = X.assert_exactly_summable(ref)
        assert 0 < units < X.EXACT_UNITS
        want = ref.exact()
        assert want.dtype == ref.dtype and torch.equal(want.double().float().double(), want.double())
        floors = ref.dtype == X.BF16 and ref.products >= MIN_PRODUCTS
        if floors:
            inexact, ties_down = X.rounding_stats(ref.ref64)
            assert inexact >= MIN_INEXACT, f"{what}: only {inexact:.3f} of the outputs are no bf16 number"
            assert ties_down >= MIN_TIES_DOWN, f"{what}: only {ties_down:.3f} of the outputs are ties rounded downward"
        mutants = ref.mutants()
        assert "one tap dropped" in mutants
        assert (ref.dtype == X.BF16) == ("truncation" in mutants) == ("round-half-away" in mutants)
        assert (ref.dtype == X.BF16 and ref.residual is not None) == ("rounded before the residual" in mutants)
        assert (ref.bias is not None) == ("bias through bf16" in mutants)
        for name, wrong in mutants.items():
            assert wrong.shape == want.shape and wrong.dtype == want.dtype
            if name in ROUNDING_MUTANTS and not floors and torch.equal(wrong, want):
                continue                    # a small output (a 1 x 1 map, eight products) may hold no value that this rounding gets wrong
            assert not torch.equal(wrong, want), f"{what}: the mutant '{name}' gives the right answer"
            with pytest.raises(AssertionError, match="elements differ"):
                X.assert_bits(wrong, want)


def test_every_listed_family_has_its_cases():
    assert len(X.FAMILIES) == 19 and all(cases for _, cases, _, _ in X.FAMILIES)
    assert sum(len(cases) for _, cases, _, _ in X.FAMILIES) == len(CASES) == 53


def test_generators_are_seeded_and_on_their_grids():
    g = X.generator("k", (1, 2))
    a = X.integers(g, 1000)
    assert torch.equal(a, X.integers(X.generator("k", (1, 2)), 1000)) and not torch.equal(a, X.integers(X.generator("k", (1, 3)), 1000))
    assert a.min() == -8 and a.max() == 8 and torch.equal(a, a.round())
    w = X.weights(g, 1000)
    assert w.abs().max() == 0.5 and torch.equal(w * 8, (w * 8).round()) and torch.equal(w.float().bfloat16().double(), w)
    b = X.biases(g, 1000)
    assert 32 < b.abs().min() and b.abs().max() < 128 and torch.equal(b * 8, (b * 8).round()) and b.min() < 0 < b.max()
    assert (b.float().bfloat16().double() != b).all()                          # a bias taken through bf16 shows: none is a bf16 number
    lo = X.lowres(g, 2, 3, 5, 4)
    up = X.enlarge2x(lo)
    assert torch.equal(lo / 16, (lo / 16).round()) and torch.equal(up, up.round()) and up.abs().max() <= 128
    assert torch.equal(up.float().bfloat16().double(), up)                     # the enlarged feature is made of bf16 numbers
    # the restated 2x enlargement, written out at one interior and one border pixel
    assert up[0, 0, 3, 3] == (9 * lo[0, 0, 1, 1] + 3 * lo[0, 0, 1, 2] + 3 * lo[0, 0, 2, 1] + lo[0, 0, 2, 2]) / 16
    assert up[0, 0, 0, 0] == lo[0, 0, 0, 0] and up[0, 0, 0, 1] == (3 * lo[0, 0, 0, 0] + lo[0, 0, 0, 1]) / 4


def test_rounding_helpers():
    f = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, -1.01171875, 1.005, -1.005, 257.0, 0.0])
    #                  exact  tie (even below)  tie (odd below)                        above the tie, below (257: tie between 256 and 258)
    assert X.round_once(f.double(), X.BF16).tolist() == [1.0, 1.0, 1.015625, -1.0, -1.015625, 1.0078125, -1.0078125, 256.0, 0.0]
    assert X.truncate_to_bf16(f).tolist() == [1.0, 1.0, 1.0078125, -1.0, -1.0078125, 1.0, -1.0, 256.0, 0.0]
    assert X.half_away_to_bf16(f).tolist() == [1.0, 1.0078125, 1.015625, -1.0078125, -1.015625, 1.0078125, -1.0078125, 258.0, 0.0]
    inexact, ties_down = X.rounding_stats(f.double())
    assert inexact == pytest.approx(7 / 9) and ties_down == pytest.approx(3 / 9)
    assert X.round_once(f.double(), X.F32) is not None and torch.equal(X.round_once(f.double(), X.F32), f)
    with pytest.raises(AssertionError, match="not an fp32 number"):
        X.round_once(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), X.BF16)


def test_the_bound_and_the_grid_are_enforced():
    x, w = torch.full((1, 64, 3, 3), 2.0 ** 10, dtype=torch.float64), torch.full((64, 64, 3, 3), 2.0 ** 5, dtype=torch.float64)
    with pytest.raises(AssertionError, match="2\\^24"):
        X.assert_exactly_summable(X.Ref(X.conv, x, w))                 # 576 products of 2^15 = 2^27.2 eighths
    with pytest.raises(AssertionError, match="not on the grid"):
        X.assert_exactly_summable(X.Ref(X.conv, x[:, :1] / 2 ** 10, w[:1, :1] / 2 ** 9))        # nine products of 1/16
    with pytest.raises(AssertionError, match="bias is not on the grid"):
        X.assert_exactly_summable(X.Ref(X.conv, x / 2 ** 10, w / 2 ** 5, bias=torch.full((1, 64, 1, 1), 1 / 16, dtype=torch.float64)))


def test_assert_bits_reports_where_and_how_far():
    want = torch.tensor([[1.0, 2.0], [300.0, -4.0]]).bfloat16()
    got = want.clone()
    X.assert_bits(got, want)
    got[1, 0], got[0, 1] = 304.0, 2.015625
    with pytest.raises(AssertionError) as e:
        X.assert_bits(got, want)
    msg = str(e.value)
    assert "2 of 4 elements differ" in msg and "(0, 1): got 2.015625 want 2.0" in msg and "(1, 0): got 304.0 want 300.0" in msg
    assert "largest difference 2 units" in msg
    with pytest.raises(AssertionError):
        X.assert_bits(want.float(), want)                              # the type is part of the answer


def test_the_gap_the_old_criterion_left():
    """conv_bias_act 64 -> 64 at (3, 64, 9, 11, 64), bias and residual, no ReLU: the output with ONE x*w product missing and the output
    truncated to bf16 both satisfy |got - ref| <= 2^-7 * max(1, |ref|.max()), the criterion of tests/test_kpff_argmax_gpu.py; neither
    survives assert_bits."""
    ref = X.conv_refs(X.conv_operands(X.CONV_C64[0]))[(False, True)]
    want, mutants = ref.exact(), ref.mutants()
    mutants["one tap dropped"] = X.round_once(ref.one_tap_dropped(smallest=True), X.BF16)       # a weight of 1/8: the hardest tap to see
    old =lambda got: (got.double() - ref.ref64).abs().max().item() <= 2.0 ** -7 * max(1.0, ref.ref64.abs().max().item())
    assert old(want)
    for name in ("one tap dropped", "truncation"):
        assert old(mutants[name]), name
        with pytest.raises(AssertionError, match="elements differ"):
            X.assert_bits(mutants[name], want)
