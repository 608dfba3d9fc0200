"""Host nibble packer of the packed H2D transfer (src/gpu/text_pack.h) through
its Python bindings: pack -> CPU reference unpack round trips, every SIMD path
the host supports against the scalar path byte for byte, exception blocks and
the 3/4 size rule.  tests/cpp/unittest_text_pack.cc covers the same packer
natively (also under the sanitizers); this file covers the bindings the GPU
tests rely on, and the synthetic data the benchmark runs on."""
import struct

import pytest

from dmlc_core_amd import data

SCALAR, AVX2, AVX512 = 1, 2, 3
SIZES = [0, 1, 2, 255, 256, 257, 511, 513, 5003]
SYMBOLS = b"0123456789:. \n-e"


def clean_text(n, seed=1):
    x = (seed * 2654435761 + 12345) & 0xFFFFFFFF
    out = bytearray(n)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = SYMBOLS[(x >> 24) % 16]
    return bytes(out)


def header(packed):
    n, nexc, _ = struct.unpack_from("<QII", packed, 0)
    return n, nexc, packed[16:32]


def check(text, want_exc, fmt="libsvm", delimiter=","):
    ref = data.pack_text(text, fmt, delimiter, ratio=-1, isa=SCALAR)
    assert ref is not None
    n, nexc, alphabet = header(ref)
    assert (n, nexc) == (len(text), want_exc)
    assert data.unpack_text_reference(ref) == text
    for isa in (0, AVX2, AVX512):
        if data.pack_isa_supported(isa):
            assert data.pack_text(text, fmt, delimiter, ratio=-1, isa=isa) == ref, isa
    return alphabet


@pytest.mark.parametrize("n", SIZES)
def test_round_trip_without_exceptions(n):
    assert check(clean_text(n, n), 0) == SYMBOLS


@pytest.mark.parametrize("n", SIZES)
def test_every_block_an_exception(n):
    t = bytearray(clean_text(n, 7))
    for b in range((n + 255) // 256):
        t[min(n - 1, b * 256 + (b * 37) % 256)] = ord("q")
    check(bytes(t), (n + 255) // 256)


@pytest.mark.parametrize("n", [1, 257, 511, 513, 5003])
def test_exception_only_in_short_last_block(n):
    t = bytearray(clean_text(n, 9))
    t[n - 1] = 9  # \t
    check(bytes(t), 1)


@pytest.mark.parametrize("byte", [0x80, 0xB0, 0xFF, 0x0D, 0x00, 0x09, ord("q"), ord("+")])
def test_exotic_bytes(byte):
    for pos in (0, 63, 64, 255, 300, 767):
        t = bytearray(clean_text(1024, 11))
        t[pos] = byte
        check(bytes(t), 1)


def test_csv_alphabet_carries_the_delimiter():
    t = clean_text(2048, 17).replace(b":", b"|")
    alphabet = check(t, 0, "csv", "|")
    assert alphabet == SYMBOLS.replace(b":", b"|")
    check(t.replace(b"|", b","), 8, "csv", "|")  # ',' in every block, not the delimiter here


def test_three_quarter_rule_both_sides():
    n = 64 * 1024
    for nexc, packs in ((62, True), (63, False)):
        # 32 + (n/2 + 16) + pad16(4 nexc) + 256 nexc <= 3n/4 holds up to nexc = 62
        t = bytearray(clean_text(n, 19))
        for b in range(nexc):
            t[b * 256 + 5] = ord("x")
        p = data.pack_text(bytes(t), "libsvm", ",")
        assert (p is not None) == packs
        if packs:
            assert len(p) <= n * 3 // 4
            assert data.unpack_text_reference(p) == bytes(t)
    assert data.pack_text(clean_text(64), "libsvm", ",") is None


@pytest.mark.parametrize("fmt", ["libsvm", "libfm", "csv"])
def test_uniform_synthetic_text_has_no_exceptions(tmp_path, fmt):
    """the benchmark's default shape packs to about half its size"""
    p = str(tmp_path / ("u." + fmt))
    data.write_synthetic(p, 0, 3000, format=fmt, seed=2)
    with open(p, "rb") as f:
        text = f.read()
    packed = data.pack_text(text, fmt, ",")
    assert packed is not None
    assert header(packed)[1] == 0
    assert len(packed) <= len(text) // 2 + 64
    assert data.unpack_text_reference(packed) == text
