"""Host models behind tests/test_flat_bf16_image_gpu.py (no GPU): the numpy restatement of the image's bf16 rounding against
plain integer arithmetic, the restated margin coefficients against the constants in csrc/flat_filter.hip, and a check that
the adversarial inputs of the margin audit really use the bound -- an audit that passes on slack alone proves nothing."""
import re
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import bf16_image_cases as BC  # noqa: E402

SRC = (ROOT / "valkey-search_amd" / "csrc" / "flat_filter.hip").read_text()


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _rne_int(u):
    """round the 32 bits of an f32 to its upper 16, nearest even, with nothing but int comparisons"""
    hi, lo = u >> 16, u & 0xFFFF
    if lo > 0x8000 or (lo == 0x8000 and (hi & 1)):
        hi += 1
    return hi & 0xFFFF


MIDPOINT_BITS = [
    0x3F808000,   # 1 + 2^-8: midpoint, kept bit even -> down to 0x3F80
    0x3F818000,   # midpoint, kept bit odd -> up to 0x3F82
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # one ulp of f32 on either side of both
    0xBF808000, 0xBF818000, 0xBF808001, 0xBF817FFF,   # the same, negative
    0x3FFF8000,   # 1.9921875 (the largest bf16 below 2) + half an ulp, kept bit odd: the carry runs into the exponent -> 2.0 = 0x4000
    0x3FFFFFFF,   # just below 2.0
    0x00000000, 0x80000000,   # +-0
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,   # f32 subnormals (midpoints among them)
    0x7F7FFFFF,   # the largest finite f32: rounds to bf16 +inf (its tile is beyond f16 anyway)
    0x7F7F7FFF,   # the largest f32 that stays finite in bf16
    0x47000000,   # 32768
]


def test_numpy_rounding_equals_integer_arithmetic_on_the_midpoint_cases():
    u = np.array(MIDPOINT_BITS, dtype=np.uint32)
    got = BC.bf16_bits(u.view(np.float32))
    want = [_rne_int(int(b)) for b in MIDPOINT_BITS]
    assert got.tolist() == want
    # spelled out, so that a mistake shared by both restatements shows
    named = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82,
             0x3FFF8000: 0x4000, 0x00000000: 0x0000, 0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002, 0x7F7FFFFF: 0x7F80,
             0x7F7F7FFF: 0x7F7F}
    for b, w in named.items():
        assert int(BC.bf16_bits(np.array([b], np.uint32).view(np.float32))[0]) == w, hex(b)
    assert _f32_bits(1.0 + 2.0 ** -8) == 0x3F808000 and _f32_bits(1.9921875 + 2.0 ** -8) == 0x3FFF8000


def test_numpy_rounding_is_round_to_nearest_even_on_random_bits():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]                       # finite
    x = u.view(np.float32)
    r = BC.bf16_round(x).astype(np.float64)
    lo = ((u & 0xFFFF0000).view(np.float32)).astype(np.float64)                      # truncation: the neighbour towards zero
    hi = ((u & 0xFFFF0000) + np.uint32(0x10000)).view(np.float32).astype(np.float64)  # the neighbour away from zero (may be inf)
    xd = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nearest = np.where(np.abs(xd - lo) < np.abs(hi - xd), lo, hi)
    tie = np.abs(xd - lo) == np.abs(hi - xd)
    even = np.where(((u >> 16) & 1) == 0, lo, hi)
    want = np.where(tie, even, nearest)
    fin = np.isfinite(hi)
    assert (r[fin] == want[fin]).all()
    # |x^ - x| <= u |x| -- or, among bf16's subnormals (spacing 2^-133), half a spacing: far inside the 2^-25 per element that
    # the margin's subnormal term charges for f16's
    assert (np.abs(r[fin] - xd[fin]) <= np.maximum(BC.U * np.abs(xd[fin]), 2.0 ** -134)).all()


def test_restated_margin_constants_are_the_ones_in_the_source():
    m = re.search(r"const float rel = a\.img_bf16 \? \((0x1p-7f) \+ (0x1p-16f)\) \+ 0x1p-22f \+ (1\.01f) \* D \* 0x1p-22f \+ \(D / 16\.f \+ 5\.f\) \* 0x1p-24f\s*"
                  r": \(a\.qbf16 \? (0x1p-8f) : a\.bf16 \? (0x1p-11f) : (0x1p-10f)\) \+ 0x1p-22f \+ D \* 0x1p-22f \+ \(D / 16\.f \+ 5\.f\) \* 0x1p-24f;", SRC)
    assert m, "the expression of `rel` in flat_qprep_kernel changed: restate it in tests/helpers/bf16_image_cases.py"
    assert float.fromhex(m.group(1).rstrip("f")) + float.fromhex(m.group(2).rstrip("f")) == BC.REL_BF16_IMAGE == 2 * BC.U + BC.U ** 2
    assert float(m.group(3).rstrip("f")) == 1.01 >= (1 + BC.U) ** 2
    assert float.fromhex(m.group(4).rstrip("f")) == BC.REL_BF16_INDEX == BC.U
    assert float.fromhex(m.group(6).rstrip("f")) == BC.REL_F16
    assert "const float sub = 0x1.01p-25f * sqrtf(D);" in SRC
    assert "c1 = (qn * rel + sub + 0x1p-23f * qn) * 1.001f, c0 = (sub * qn + 0x1p-23f) * 1.001f;" in SRC
    # the image's rounding is the query fragments' expression
    assert SRC.count("(u + 0x7FFFu + ((u >> 16) & 1u)) >> 16") == 2


@pytest.mark.parametrize("side", [1, -1])
@pytest.mark.parametrize("dim,dp", [(64, 64), (192, 192), (768, 768), (100, 128)])
@pytest.mark.parametrize("log2_norm", [-10, 0, 10])
def test_adversarial_inputs_use_the_bound(dim, dp, log2_norm, side):
    """|x^.q^ - x.q| in float64 against E_q(|x|) of the restated coefficients.  Both roundings at u / (1 + u) give (2u - u^2) |x||q|
    nearly; the relative part of the bound is (2u + u^2 + 1.01 D 2^-22 + ...) |x||q|: 0.97 of it is reached at D = 768, more
    below, and 0.9 of the WHOLE bound is asked at row norms 1 and 2^10.  At row norm 2^-10 and below (rows r % 3 != 0 are 2 and
    4 times shorter still) the absolute terms of the bound -- c0 = (2^-25 sqrt(D) |q| + 2^-23) 1.001 and 2^-25 sqrt(D) R, which
    no input of this size can use -- are up to 0.4 of it (printed below): there 0.9 of the bound's relative part, |q| rel R, is
    asked, which is the part the two roundings answer for."""
    X, Q = BC.adversarial(6, 4, dim, dp, side, log2_norm, seed=dim)
    xh, qh = BC.bf16_round(X).astype(np.float64), BC.bf16_round(Q).astype(np.float64)
    xd, qd = X.astype(np.float64), Q.astype(np.float64)
    assert ((xh - xd) * np.sign(xd) * side >= 0).all() and (np.abs(xh - xd)[:, :dim] > 0.99 * BC.U / (1 + BC.U) * np.abs(xd)[:, :dim]).all()
    err = np.abs(xh @ qh.T - xd @ qd.T)
    R = np.linalg.norm(xd, axis=1)
    assert 2.0 ** (log2_norm - 0.6) < R.max() < 2.0 ** (log2_norm + 0.6)
    c1, c0 = BC.margin_coefs(np.linalg.norm(qd, axis=1) * 1.0001, dp, BC.REL_BF16_IMAGE, 1.01)
    E = c1[None, :] * R[:, None] + c0[None, :]
    use = err / E
    assert (use <= 1.0).all(), use.max()
    if log2_norm >= 0:
        assert use.min() >= 0.9, use.min()
    else:
        qn = np.linalg.norm(qd, axis=1) * 1.0001
        rel = BC.REL_BF16_IMAGE + 2.0 ** -22 + 1.01 * dp * 2.0 ** -22 + (dp / 16.0 + 5.0) * 2.0 ** -24
        print("use of the whole bound at row norm 2^%d: %.3f .. %.3f" % (log2_norm, use.min(), use.max()))
        assert (err >= 0.9 * 1.001 * rel * qn[None, :] * R[:, None]).all()
    # half the bound (the row term left out, or r03's 2^-9 for 2^-8) is NOT enough for these inputs (at norms where the
    # absolute terms do not pay for it)
    c1h, c0h = BC.margin_coefs(np.linalg.norm(qd, axis=1) * 1.0001, dp, BC.REL_BF16_INDEX, 1.0)
    if log2_norm >= 0:
        assert (err > c1h[None, :] * R[:, None] + c0h[None, :]).all()
