"""CPU-side checks of the device writer of the kNN export (include/cdml_knn_writer.h, csrc/knn_writer.hip): the shortest-repr
routine -- the SAME __host__ __device__ code the kernels run, through its host entry point cdml_f32_shortest -- against
numpy's str of a float32 on millions of values and on every edge the routine has (powers of two, where the float below is
half as far; neighbours of short decimals; the switch to scientific layout at 1e-4; the carry out of a run of nines; both ends
of the stated range), header == binding table == library, and the argument errors of the two launches (before any HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = np.float32(2.0 ** -64), np.float32(2.0)           # the routine's range [LO, HI), as the header states it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cdml_amd import _lib
    return _lib.load_library()


def shortest(lib, x):
    """the routine's text for every element of x (float32), '' where it refuses"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    buf = C.create_string_buffer(16)
    out = []
    for v in x.tolist():
        n = lib.cdml_f32_shortest(C.c_float(v), buf)
        out.append(buf.value.decode() if n >= 0 else "")
        assert n == (len(out[-1]) if n >= 0 else -1) and n <= 14
    return np.array(out)


def assert_numpy(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    x = x[(x >= LO) & (x < HI)]
    got, want = shortest(lib, x), x.astype(str)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(x[i].view(np.uint32), got[i], want[i]) for i in bad[:8]]
    return len(x)


def test_two_million_random_values_equal_numpy(lib):
    rng = np.random.RandomState(0)
    n = assert_numpy(lib, np.exp(rng.uniform(np.log(1e-7), np.log(1.4), 1000000)))       # log-uniform over (1e-7, 1.4)
    n += assert_numpy(lib, rng.uniform(0.0, 1.4, 1000000))                                  # uniform over (0, 1.4)
    n += assert_numpy(lib, np.exp(rng.uniform(np.log(float(LO)), np.log(2.0), 100000)))    # the whole stated range
    assert n >= 2000000


def test_powers_of_two_and_dyadic_fractions(lib):
    """2^-j: the significand is 2^23, the float below is half as far as the one above (unequal margins); k / 2^j"""
    assert assert_numpy(lib, 2.0 ** -np.arange(0, 65, dtype=np.float64)) == 65
    ks = np.arange(1, 64, dtype=np.float64)
    x = np.concatenate([ks / 2.0 ** j for j in range(0, 40)])
    assert assert_numpy(lib, x) > 2000
    assert shortest(lib, [0.5, 0.25, 1.0, 1.25, 1.5, 2.0 ** -10]).tolist() == ["0.5", "0.25", "1.0", "1.25", "1.5", "0.0009765625"]


def test_neighbours_of_short_decimals(lib):
    """b 10^-a for a <= 9, b < 100: the decimal itself, and the floats just below and above it (which need 8 or 9 digits)"""
    dec = np.array([b * 10.0 ** -a for a in range(0, 10) for b in range(1, 100)]).astype(np.float32)
    n = assert_numpy(lib, dec)
    n += assert_numpy(lib, np.nextafter(dec, np.float32(0)))
    n += assert_numpy(lib, np.nextafter(dec, np.float32(4)))
    assert n > 2400
    assert shortest(lib, np.nextafter(np.float32(0.3), np.float32(1)))[0] == "0.30000004"


def test_layout_switch_at_1e_minus_4_and_the_keep_threshold(lib):
    a = np.float32(1e-4)                                          # 9.99999974737875e-05: below 1e-4, so scientific
    below, above = np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(1))
    assert shortest(lib, [below, a, above, 1e-5, 9.999e-5, 0.00012345]).tolist() == \
        ["9.999999e-05", "1e-04", "0.000100000005", "1e-05", "9.999e-05", "0.00012345"]
    x = a
    near = [a]
    for _ in range(64):
        x = np.nextafter(x, np.float32(1))
        near.append(x)
    x = a
    for _ in range(64):
        x = np.nextafter(x, np.float32(0))
        near.append(x)
    t = np.float32(1.4)                                           # the writer keeps d < 1.4f: the floats around it
    x = t
    near.append(t)
    for _ in range(64):
        x = np.nextafter(x, np.float32(0))
        near.append(x)
    x = t
    for _ in range(8):
        x = np.nextafter(x, np.float32(2))
        near.append(x)
    assert assert_numpy(lib, np.array(near)) == len(near)
    # a carry into a run of nines shortens the digits (1.29999995... -> 1.3); out of it, it moves the decade (9.99999975e-05 -> 1e-04)
    assert shortest(lib, [np.float32(1.3), a, np.nextafter(np.float32(1), np.float32(0))]).tolist() == ["1.3", "1e-04", "0.99999994"]


def test_both_ends_of_the_stated_range(lib):
    text = open(os.path.join(ROOT, "include", "cdml_knn_writer.h")).read()
    assert "#define CDML_F32_SHORTEST_MIN 0x1p-64f" in text and "#define CDML_F32_SHORTEST_MAX 2.0f" in text
    assert "#define CDML_F32_SHORTEST_CHARS 14" in text
    top = np.nextafter(HI, np.float32(0))
    assert shortest(lib, [LO, top]).tolist() == [str(LO), str(top)] == ["5.421011e-20", "1.9999999"]
    assert assert_numpy(lib, [LO, np.nextafter(LO, np.float32(1)), top, np.nextafter(top, np.float32(0))]) == 4
    buf = C.create_string_buffer(b"untouched", 16)
    for x in (np.nextafter(LO, np.float32(0)), HI, 0.0, -0.5, 1e-30, 1e-45, np.inf, -np.inf, np.nan, 3.0):
        assert lib.cdml_f32_shortest(C.c_float(x), buf) == -1 and buf.value == b"untouched"
    assert lib.cdml_f32_shortest(C.c_float(0.5), None) == -1
    # [1e-4, 1.4) -- the positional part of what the writer keeps -- lies inside
    assert LO < np.float32(1e-4) and np.float32(1.4) < HI


def test_header_equals_binding_table_equals_library(lib):
    from cdml_amd import _lib
    text = open(os.path.join(ROOT, "include", "cdml_knn_writer.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    abi = text[text.index('extern "C" {'):text.index("#ifdef __cplusplus\n}")]
    syms = sorted(set(re.findall(r"\b(cdml_[a-z0-9_]+)\s*\(", abi)))
    assert syms == sorted(_lib.SIGNATURES_KNN_WRITER) == ["cdml_f32_shortest", "cdml_knn_line_sizes", "cdml_knn_line_write"]
    for s in syms:
        assert getattr(lib, s).argtypes == _lib.SIGNATURES_KNN_WRITER[s][1]
        n_args = abi[abi.index(s + "("):].split(")")[0].count(",") + 1
        assert n_args == len(_lib.SIGNATURES_KNN_WRITER[s][1]), s
    others = [getattr(_lib, t) for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_KNN_WRITER"]
    assert len(others) >= 11 and not any(set(syms) & set(t) for t in others)
    main = open(os.path.join(ROOT, "include", "cdml.h")).read()
    assert not set(syms) & set(re.findall(r"\b(cdml_\w+)\s*\(", main))


def test_argument_errors_come_before_any_hip_call(lib):
    p = C.c_void_p(4096)

    def sizes(D=p, ldd=8, I=p, ldi=8, row0=0, n=10, k=8, goff=p, n_guid=10, total=100, out=p, flags=p):
        return lib.cdml_knn_line_sizes(D, ldd, I, ldi, row0, n, k, goff, n_guid, total, out, flags, None)

    def write(D=p, ldd=8, I=p, ldi=8, row0=0, n=10, k=8, gb=p, goff=p, n_guid=10, total=100, off=p, out=p, nbytes=64):
        return lib.cdml_knn_line_write(D, ldd, I, ldi, row0, n, k, gb, goff, n_guid, total, off, out, nbytes, None)

    for f in (sizes, write):
        for kw in (dict(D=None), dict(I=None), dict(goff=None), dict(n=0), dict(n=-3), dict(row0=-1), dict(total=-1),
                   dict(ldd=7), dict(ldi=7), dict(row0=1), dict(n_guid=9)):
            assert f(**kw) == -1, kw
            assert f.__name__ in lib.cdml_last_error().decode() or "knn_line_" in lib.cdml_last_error().decode()
        assert f(k=0) == -4 and f(k=129, ldd=129, ldi=129) == -4
        assert b"k must be in [1, 128]" in lib.cdml_last_error()
    assert sizes(out=None) == -1 and sizes(flags=None) == -1
    assert write(off=None) == -1 and write(out=None) == -1 and write(gb=None) == -1 and write(nbytes=-1) == -1
    assert b"out_bytes" in lib.cdml_last_error()
    assert sizes(row0=5, n=5, n_guid=9) == -1 and b"have no guid" in lib.cdml_last_error()


def test_guid_table_is_utf8_bytes_and_offsets(lib):
    from cdml_amd import knn
    names = ["a", "", "éè", "漢字", "\U0001f600", "tail"]
    gb, go = knn.guid_table(names, device="cpu")
    assert go.tolist() == [0, 1, 1, 5, 11, 15, 19] and gb.numel() == 20
    assert bytes(gb[:19].tolist()) == "".join(names).encode("utf-8")
    gb2, go2 = knn.guid_table(dict(enumerate(names)), device="cpu")
    assert gb2.tolist() == gb.tolist() and go2.tolist() == go.tolist()
    g0, o0 = knn.guid_table([], device="cpu")
    assert o0.tolist() == [0] and g0.numel() == 1
    with pytest.raises(ValueError, match="keys 0 .. 1"):
        knn.guid_table({0: "a", 5: "b"}, device="cpu")
