"""Host models and inputs shared by tests/test_flat_bf16_image_model_cpu.py and tests/test_flat_bf16_image_gpu.py: the bf16
rounding of the row image (row_stats_kernel, option flat-image-format = 1) restated in numpy, the margin coefficients of
flat_qprep_kernel restated in float64, and the inputs that drive both roundings of a product against the margin."""
import numpy as np

U = 2.0 ** -8                      # unit roundoff of bf16 (8 significant bits)
REL_BF16_IMAGE = 2.0 ** -7 + 2.0 ** -16   # (2u + u^2): f32 rows behind a bf16 image, both operands rounded
REL_BF16_INDEX = 2.0 ** -8                # bf16 rows: the query alone
REL_F16 = 2.0 ** -10                      # f32 rows through f16, both operands at 2^-11


def bf16_bits(x):
    """round to nearest even, the integer expression of the kernels: (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the f32 bits"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def margin_coefs(qn_up, D, rel_operands, acc_factor=1.0):
    """(c1, c0) of the inner-product space as flat_qprep_kernel builds them (float64, without its f32 rounding): qn_up = |q| *
    1.0001, D = the padded dimension; rel_operands = the rounding of the two operands, acc_factor = what the accumulation term
    is multiplied with (1.01 behind a bf16 image)."""
    rel = rel_operands + 2.0 ** -22 + acc_factor * D * 2.0 ** -22 + (D / 16.0 + 5.0) * 2.0 ** -24
    sub = (1.0 + 2.0 ** -8) * 2.0 ** -25 * np.sqrt(D)          # 0x1.01p-25f * sqrt(D)
    c1 = (qn_up * rel + sub + 2.0 ** -23 * qn_up) * 1.001
    c0 = (sub * qn_up + 2.0 ** -23) * 1.001
    return c1, c0


def adversarial(n, nq, dim, dp, side, log2_norm=0, seed=0):
    """Every element of every row AND every query just past a bf16 rounding midpoint (tests/helpers/exp_margin_check.py has the
    queries there; here both operands are rounded): magnitude 2^e (1 + 2^-8 +- 2^-20) -- `side` +1: just above the midpoint
    between 2^e and 2^e (1 + 2^-7), rounds UP by nearly half an ulp; -1: just below, rounds DOWN by as much -- so the relative
    error of an element is the largest bf16 has, u / (1 + u).  One sign vector for rows and queries: every product is positive,
    all rows are parallel to all queries (Cauchy-Schwarz is tight), and the two roundings of every product err the same way --
    all errors add.  Row r is scaled by 2^-(r % 3), query j by 2^-(j % 2) (powers of two keep the midpoints), so that scores
    differ; e is chosen for a row norm of about 2^log2_norm (within sqrt 2).
    -> rows [n][dp], queries [nq][dp] f32, zero beyond dim."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    m = 1.0 + 2.0 ** -8 + side * 2.0 ** -20
    e = int(np.round(log2_norm - 0.5 * np.log2(dim)))
    X = np.zeros((n, dp), np.float32)
    Q = np.zeros((nq, dp), np.float32)
    X[:, :dim] = (s * m)[None, :] * (2.0 ** (e - np.arange(n) % 3))[:, None]
    e_q = int(np.round(-0.5 * np.log2(dim)))
    Q[:, :dim] = (s * m)[None, :] * (2.0 ** (e_q - np.arange(nq) % 2))[:, None]
    assert (X.astype(np.float64)[:, :dim] == (s * m)[None, :] * (2.0 ** (e - np.arange(n) % 3))[:, None]).all()   # exact in f32
    return X, Q
