"""The placed LibSVM / LibFM cases of svm_cases.py on the host: the C++ parsers
(src/data/libsvm_parser.h, libfm_parser.h) equal the Python oracle
(pyref.parse_libsvm / parse_libfm) bit for bit on every case, which is what
lets test_gpu_svm_edges.py hold the HIP kernels to the C++ parser; and the
generator's own bookkeeping: every claim of a case holds on the model of the
walk, every marked byte is at its offset, every file is below 64 KiB, and the
model of what leaves the tile path agrees with what every case expects."""
import numpy as np
import pytest

from dmlc_core_amd import data
import svm_cases as sc
import pyref

GROUP_FORMATS = [(g, f) for g in sc.GROUPS for f in sc.FORMATS]


def cpu_rows(uri, fmt, index64=False):
    return pyref.concat_blocks(list(data.iter_blocks(uri, type=fmt, index64=index64)))


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_cpu_parser_equals_the_oracle(tmp_path, group, fmt):
    for case in sc.cases(group, fmt):
        p = sc.write(case, str(tmp_path / f"{case.name}.{fmt}"))
        for index64 in ((False, True) if group in sc.INDEX64_GROUPS else (False,)):
            got = cpu_rows(p, fmt, index64)
            msg = sc.first_difference(case, got, sc.oracle(case, index64))
            assert not msg, f"index64={index64}: {msg}"


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_cases_hold_what_they_claim(group, fmt):
    cases = sc.cases(group, fmt)
    assert cases
    for case in cases:
        assert len(case.text) < sc.MAX_FILE, case.name
        assert case.expect in ("tile", "exact", "either") and case.hexpect in ("tile", "exact", "either")
        assert case.expect != "either" or case.name in sc.EITHER
        for off, ch in case.marks:
            assert case.text[off] == ch, (case.name, off)
        assert not any(ord(c) < 32 and c not in "\t\r\n" for c in case.text), case.name
        said = sc.check_claims(case.text, fmt, case.claims)
        assert len(said) == len(case.claims)
        assert (case.expect == "exact") == bool(sc.exact_reasons(case.text, fmt)), case.name
        assert (case.hexpect == "exact") == bool(sc.exact_reasons(case.text, fmt, True)), case.name
        assert case.dyadic == (group in sc.DYADIC_GROUPS) or "token" in case.name or group == "g"
        if group == "e" and case.expect == "tile":
            # the non-lean fill: every case has a weight or a qid
            rows = sc.oracle_rows(case.text, fmt)
            assert any(r[1] is not None or (fmt == "libsvm" and r[2] is not None) for r in rows)


def test_the_model_on_a_text_small_enough_to_count_by_hand():
    """two tiles: 70 one-token lines, a long line over the tile edge, 3 tokens"""
    text = "1\n" * 70 + "1 " + "5:1 " * 40 + "\n"
    text += "0" + " " * (sc.TILE + 100 - len(text) - 1) + "7:1 8:1\n1 2:1\n"
    fill = sc.fill_model(text, "libsvm")
    s0 = fill[0, 0]
    assert (s0.ntok, s0.nline, s0.total, s0.rest, s0.ndec, s0.carry) == (112, 72, 112, 48, 64, 48)
    s1 = fill[0, 1]
    assert (s1.ntok, s1.carry_in, s1.total, s1.rest, s1.ndec) == (0, 48, 48, 0, 48)
    assert fill[1, 0].ntok == 4 and fill[1, 0].nline == 1 and fill[1, 0].carry == 4
    assert fill[1, 1].ndec == 4  # a step without tokens decodes what it was handed
    h = sc.hash_model(text, "libsvm")
    assert h[0].own == 72 and h[1].own == 1
    # tile 0 follows its last line into tile 1 and stops at the line start there
    assert len(h[0].steps) == sc.STEPS + 1 and h[0].steps[-1].last
    assert h[0].steps[-1].ntok_a == 2  # `7:1 8:1`: the next line's tokens are not owned
    assert h[0].steps[0].carry == 0    # the first left-over token starts before byte 1024
    assert h[1].steps[0].ntok_a == 2 and h[1].steps[0].last
    assert sc.defers("3:1.5e0001") and sc.defers("3:0.1234567890123456") and sc.defers("3:12345678.5")
    assert not sc.defers("3:1.5e-3") and not sc.defers("12:0.123456789012345")


def test_the_placements_are_where_the_kernels_have_their_edges():
    """spot checks of the plan itself: every edge, distance, length and round
    total that the groups promise is among the built cases"""
    by = {(c.name, f): c for g in sc.GROUPS for f in sc.FORMATS for c in sc.cases(g, f)}
    for fmt in sc.FORMATS:
        # a, b: a mark on or next to every edge
        for name, d in (("a_nl_m2", -2), ("a_nl_m1", -1), ("a_nl_0", 0), ("a_nl_p1", 1),
                        ("b_feature_0", -1), ("b_feature_1", 0), ("b_feature_2", 1),
                        ("b_label_0", -1), ("b_label_1", 0), ("b_label_2", 1)):
            at = [off - d for off, ch in by[name, fmt].marks if ch != "\n" or name[0] == "a"]
            assert at == list(sc.EDGES), name
        # c: every (step end, k, length), own and carried
        seen = set()
        for case in sc.cases("c", fmt):
            model = sc.fill_model(case.text, fmt)
            for c in case.claims:
                if c[0] != "last_tok":
                    continue
                _, t, s, off = c
                end = t * sc.TILE + (s + 1) * sc.STEP
                tok = case.text[off:].split()[0]
                seen.add((s, end - off, len(tok), model[t, s].carry > 0))
        floor = 1 if fmt == "libsvm" else 3
        want = {(s, k, n, carried) for carried in (False, True)
                for s in range(sc.STEPS - carried) for k in sc.C_BACK
                for n in {k + 1, *sc.C_LENGTHS} if n > k and n >= floor}
        assert seen == want
        # every shape at every distance before an edge
        shapes = {(p[1], p[3]) for p in sc.c_placements(fmt)}
        assert all((k, sh) in shapes for k in sc.C_BACK for sh in sc.C_SHAPES)
        # d: the totals, entered with and without a carry
        for name, carried in (("d_totals", False), ("d_totals_carried", True)):
            case = by[name, fmt]
            totals = [c[4] for c in case.claims if c[0] == "fill" and c[3] == "total"]
            assert totals == list(sc.D_TOTALS)
            assert any(c[3] == "carry_in" and c[4] > 0 for c in case.claims) == carried
        # g: every size with every ending
        sizes = {len(c.text) for c in sc.cases("g", fmt)}
        assert set(sc.G_SIZES) <= sizes
    # e: the qid group is LibSVM only
    assert not any("qid" in c.name or "near" in c.name for c in sc.cases("e", "libfm"))
    assert {c.name for c in sc.cases("e", "libsvm") if c.expect == "exact"} == \
        {"e_near_" + n for n in sc.E_NEAR}
    # f: the list limit splits at 429, and a half of 429 leaves the tile path
    assert not sc.hash_model(by["f_list_428", "libsvm"].text, "libsvm")[1].steps[1].split
    assert sc.hash_model(by["f_list_429", "libsvm"].text, "libsvm")[1].steps[1].split
    assert by["f_half_a_429", "libsvm"].hexpect == by["f_half_b_429", "libfm"].hexpect == "exact"


def test_first_difference_names_the_token():
    case = sc.cases("b", "libsvm")[0]
    want = sc.oracle(case)
    got = {k: (None if v is None else v.copy()) for k, v in want.items()}
    assert sc.first_difference(case, got, want) is None
    got["value"][5] += 1
    msg = sc.first_difference(case, got, want)
    assert "value[5]" in msg and "nearest mark" in msg
    assert np.array_equal(got["offset"], want["offset"])
