"""numpy reference of the fp8 catalogue's quantiser (include/cdml_f8.h): per row one power-of-two scale from the largest
finite magnitude, codes = round-to-nearest-even e4m3 of x / scale, written from the format's definition with integer
arithmetic only (no torch, no float8 type).  Plain module, no pytest configuration."""
import numpy as np


def decode(codes):
    """float64 value of every OCP e4m3fn code (uint8 array); 0x7F / 0xFF -> NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    return np.where(c & 0x80, -v, v)


def encode(y):
    """RNE e4m3fn code of float64 |y| <= 448 (uint8); a non-finite y -> the NaN code of its sign."""
    y = np.asarray(y, dtype=np.float64)
    fin = np.isfinite(y)
    a = np.where(fin, np.abs(y), 0.0)
    e = np.clip(np.frexp(a)[1] - 1, -6, 8)                  # floor(log2 a), clamped to the subnormal / top binade
    q = np.rint(np.ldexp(a, 3 - e)).astype(np.int64)        # units of 2^(e - 3): exact scaling, numpy rounds half to even
    code = np.where(q < 8, q, ((e + 7) << 3) + (q - 8))     # (q = 16 carries into the next exponent by itself)
    sign = np.where(np.signbit(y), 0x80, 0)
    return np.where(fin, code | sign, 0x7F | sign).astype(np.uint8)


def quantize(x):
    """(codes uint8 [n, F], scale float32 [n]) of a float [n, F] array."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = np.where(np.isfinite(x), np.abs(x), 0.0).max(axis=1, initial=0.0)
    k = np.where(m > 0, np.maximum(np.frexp(m)[1] - 1, -119) - 7, 0)
    return encode(np.ldexp(x, -k[:, None])), np.ldexp(1.0, k).astype(np.float32)


def error_bound(x, scale):
    """The format's per-row bound on |dequantised - x|_2: 2^-4 |x|_2 + sqrt(F) 2^-10 scale (finite rows)."""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 ** -4 * np.linalg.norm(x, axis=1) + np.sqrt(x.shape[1]) * 2.0 ** -10 * np.asarray(scale, dtype=np.float64)


def sample_rows(F, n=300, seed=0):
    """The quantiser tests' inputs, float32 [n, F]: U[0,1), normal and heavy-tailed (randn^5) rows in turn, and among them a
    zero row, a one-element row, a row whose maximum is a power of two and one just below it (its code rounds up to 256),
    rows around 1e-20, in the fp32 denormals and near the fp32 maximum, negative rows, and a row with Inf and NaN elements
    of both signs."""
    rng = np.random.default_rng(seed + F)
    x = np.empty((n, F), dtype=np.float32)
    x[0::3] = rng.random((len(x[0::3]), F))
    x[1::3] = rng.standard_normal((len(x[1::3]), F))
    x[2::3] = rng.standard_normal((len(x[2::3]), F)) ** 5
    u = rng.random((16, F)).astype(np.float32)
    x[3] = 0
    x[4] = 0
    x[4, 0] = 0.3
    x[5] = 0.5 * u[0]
    x[5, 1 % F] = 4.0
    x[6] = 0.5 * u[1]
    x[6, 2 % F] = np.nextafter(np.float32(4.0), np.float32(0))
    x[7] = u[2] * np.float32(1e-20)
    x[8] = -u[3]
    x[9] = -3 * np.abs(x[1])
    x[10, 0], x[10, 1 % F], x[10, 3 % F], x[10, 4 % F] = np.inf, np.nan, -np.inf, -np.float32(np.nan)
    x[11] = u[4] * np.float32(1e-42)
    x[12] = (u[5] - 0.5) * np.float32(3e38)
    x[13] = 0
    x[13, F - 1] = -1.0
    return x
