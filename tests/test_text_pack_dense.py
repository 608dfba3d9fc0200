"""The dense code of the packed H2D transfer (src/gpu/text_pack_dense.h) on
the synthetic shards, on the CPU: what it saves over the nibble code's 0.50 on
uniform text of each format, and that every shape decodes to the same bytes
whichever encoder, range size or thread count packed it."""
import pytest

from dmlc_core_amd import data

FORMATS = ("libsvm", "libfm", "csv")


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    out = {}
    for fmt in FORMATS:
        for shape in ("uniform", "mixed"):
            p = str(d / f"{shape}.{fmt}")
            data.write_synthetic(p, 0, 1200, format=fmt, seed=4, shape=shape)
            with open(p, "rb") as f:
                out[fmt, shape] = f.read()
    return out


def isas():
    return [i for i in (1, 3) if data.pack_isa_supported_dense(i)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_uniform_packs_below_the_nibble_code(texts, fmt):
    text = texts[fmt, "uniform"]
    packed = data.pack_text(text, fmt, ",", ratio=-1, code="dense")
    print(fmt, len(text), len(packed), len(packed) / len(text))
    assert data.unpack_text_reference(packed) == text
    # the nibble code gives 0.50; `:0.` (`,0.`) as one code and 2 bytes of
    # metadata per block give about 0.446
    assert len(packed) <= 0.455 * len(text)
    # and the 3/4 rule lets it through
    assert data.pack_text(text, fmt, ",", code="dense") == packed


@pytest.mark.parametrize("shape", ["uniform", "mixed"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip(texts, fmt, shape):
    text = texts[fmt, shape]
    want = None
    for isa in isas():
        for range_blocks in (1, 7, 1024):
            packed = data.pack_text(text, fmt, ",", ratio=-1, isa=isa, code="dense",
                                    range_blocks=range_blocks)
            assert data.unpack_text_reference(packed) == text
            if range_blocks == 1024:
                # every encoder writes the same bytes
                want = want or packed
                assert packed == want
    for threads in (1, 4):
        packed = data.pack_text_pool(text, fmt, ",", range_blocks=64, threads=threads)
        assert data.unpack_text_reference(packed) == text
        assert len(packed) == len(data.pack_text(text, fmt, ",", ratio=-1, code="dense",
                                                 range_blocks=64))


def test_text_outside_every_table_goes_raw():
    text = bytes((i * 7) % 251 for i in range(20000))
    assert data.pack_text(text, "libsvm", ",", code="dense") is None
    packed = data.pack_text(text, "libsvm", ",", ratio=-1, code="dense")
    assert data.unpack_text_reference(packed) == text
    assert len(packed) > len(text)


def test_nibble_code_is_unchanged(texts):
    text = texts["libsvm", "uniform"]
    packed = data.pack_text(text, "libsvm", ",", ratio=-1)
    assert packed == data.pack_text(text, "libsvm", ",", ratio=-1, code="nibble")
    assert data.unpack_text_reference(packed) == text
    assert 0.5 * len(text) <= len(packed) < 0.51 * len(text)
