"""The placed CSV cases of csv_cases.py on the host: the C++ CSV parser
(src/data/csv_parser.h) equals the Python oracle (pyref.parse_csv) bit for bit
on every case under every configuration, which is what lets
test_gpu_csv_edges.py hold the HIP kernels to the C++ parser; and the
generator's own bookkeeping: every intended byte is at its offset, every file
is below 64 KiB, and the model of what leaves the tile path (a step of more
than 512 field starts, no row start within the 4 KiB extension) agrees with
what every case says it expects."""
import numpy as np
import pytest

from dmlc_core_amd import data
import csv_cases as cc
import pyref


def cpu_rows(uri, fmt="csv", index64=False):
    return pyref.concat_blocks(list(data.iter_blocks(uri, type=fmt, index64=index64)))


GROUP_DELIMS = [(g, d) for g in cc.GROUPS for d in cc.delims(g)]


@pytest.mark.parametrize("group,delim", GROUP_DELIMS)
def test_cpu_parser_equals_the_oracle(tmp_path, group, delim):
    for case in cc.cases(group, delim):
        p = cc.write(case, str(tmp_path / f"{case.name}.csv"))
        for lc, wc in cc.configs(group):
            got = cpu_rows(p + cc.query(lc, wc, delim))
            msg = cc.first_difference(case, got, cc.oracle(case, lc, wc))
            assert not msg, f"label_column={lc} weight_column={wc}: {msg}"


@pytest.mark.parametrize("lc,wc", cc.REFUSED)
def test_cpu_parser_refuses_a_weight_column_equal_to_the_label_column(tmp_path, lc, wc):
    case = cc.cases("g")[0]
    p = cc.write(case, str(tmp_path / "g.csv"))
    with pytest.raises(Exception, match="label_column and weight_column must differ"):
        cpu_rows(p + cc.query(lc, wc, ","))


def test_oracle_weight_column_follows_the_grammar():
    text = "1,2,3\n4\n5,6,\n,\n"
    assert pyref.parse_csv(text) == [(0.0, [1.0, 2.0, 3.0]), (0.0, [4.0]), (0.0, [5.0, 6.0]),
                                     (0.0, [0.0])]
    assert pyref.parse_csv(text, 0, ",", 2) == [(1.0, [2.0], 3.0), (4.0, [], 1.0),
                                                (5.0, [6.0], 1.0), (0.0, [], 1.0)]
    assert pyref.parse_csv(text, -1, ",", 0) == [(0.0, [2.0, 3.0], 1.0), (0.0, [], 4.0),
                                                 (0.0, [6.0], 5.0), (0.0, [], 0.0)]


@pytest.mark.parametrize("group,delim", GROUP_DELIMS)
def test_cases_hold_what_they_claim(group, delim):
    cases = cc.cases(group, delim)
    assert cases
    for case in cases:
        assert len(case.text) < cc.MAX_FILE, case.name
        assert case.expect in ("tile", "exact", "either")
        assert case.expect != "either" or group == "d"
        for off, ch in case.marks:
            assert case.text[off] == ch, (case.name, off)
        assert not any(ord(c) < 32 and c not in "\t\r\n" for c in case.text), case.name
        why = cc.exact_reasons(case.text, delim)
        if case.expect == "exact":
            assert why, case.name
        elif case.expect == "tile":
            assert not why, (case.name, why)


def test_the_placements_are_where_the_kernel_has_its_edges():
    """spot checks of the geometry, by the field-start model of the walk"""
    T, S = cc.TILE, cc.STEP
    by = {c.name: c for g in cc.GROUPS for c in cc.cases(g)}
    # f: the aligned steps hold exactly the field starts their names say
    for n in (511, 512, 513, 1024):
        per_step, _ = cc.step_field_starts(by[f"f_fields_{n}_shift0"].text, ",")
        assert per_step[(T + 2 * S) // S] == n
    per_step, _ = cc.step_field_starts(by["f_fields_513_shift1"].text, ",")
    assert per_step[(T + 2 * S) // S] == 512
    per_step, _ = cc.step_field_starts(by["f_fields_514_shift1"].text, ",")
    assert per_step[(T + 2 * S) // S] == 513
    per_step, starts = cc.step_field_starts(by["f_rows_512_shift0"].text, ",")
    assert per_step[(T + 2 * S) // S] == 512
    assert ((starts >= T + 2 * S) & (starts < T + 3 * S)).sum() == 512
    # g: one row of 3000 fields, 512 field starts in each of its full steps
    g = by["g_row3000"]
    per_step, starts = cc.step_field_starts(g.text, ",")
    s0 = (T + T // 2) // S
    assert list(per_step[s0:s0 + 5]) == [512] * 5 and per_step.max() == 512
    assert len(pyref.parse_csv(g.text.split("\n")[np.searchsorted(starts, T + T // 2)])[0][1]) == 3000
    # c: a tile without a row start; the row starts the names promise
    for name in ("c_norow_end", "c_norow_end_nl", "c_norow_full"):
        _, starts = cc.step_field_starts(by[name].text, ",")
        tile = 2 if name != "c_norow_full" else 1
        assert not ((starts >= tile * T) & (starts < (tile + 1) * T)).any(), name
    _, starts = cc.step_field_starts(by["c_starts"].text, ",")
    first = [int(starts[np.searchsorted(starts, t * T)]) - t * T for t in (1, 2, 3, 4)]
    assert first[1:] == [0, S - 1, cc.LANE * 7 + 5] and T - 1 in starts
    # c: 1, 2 and 500 field starts of the previous row open the tile
    c = by["c_pre"]
    raw = np.frombuffer(c.text.encode(), np.uint8)
    _, starts = cc.step_field_starts(c.text, ",")
    for t, want in ((1, 1), (2, 2), (3, 500)):
        first_row = int(starts[np.searchsorted(starts, t * T)])
        # every field of the tail is opened by a delimiter: the one at T - 1 included
        assert (raw[t * T - 1:first_row - 1] == ord(",")).sum() == want
    # e: every size, every last byte; the suspected case ends with extension step 4
    e = cc.cases("e")
    assert len(e) == len(cc.END_SIZES) * len(cc.END_BYTES) * 2 - len(cc.END_BYTES)
    last = by[f"e_end_{T + 4 * S}_digit"]
    _, starts = cc.step_field_starts(last.text, ",")
    assert len(last.text) == 2 * T + 4 * S and T <= starts[-1] < 2 * T
    assert last.text[T + 10 * S:T + 10 * S + 32].replace(",", "").replace(".", "").isdigit()
    # h: every number at every distance 1..15 before an even and an odd step end
    seen = set()
    for case in cc.cases("h"):
        for off, ch in case.marks:
            if ch != "\n":
                k = -off % S
                seen.add((k, (off // S) % 2))
    assert seen == {(k, p) for k in range(1, 16) for p in (0, 1)}


@pytest.mark.parametrize("fmt", ["libsvm", "libfm"])
def test_chunk_end_files_of_the_token_formats(fmt):
    files = cc.svm_end_cases(fmt)
    assert len(files) == len(cc.END_SIZES) * 6
    for name, text in files:
        assert len(text) - cc.TILE in cc.END_SIZES, name
        last = text.rstrip("\r\n").rsplit("\n", 1)[1]
        assert 2900 <= len(last) <= 5500, (name, len(last))
        rows = pyref.parse_libsvm(text) if fmt == "libsvm" else pyref.parse_libfm(text)
        assert len(rows) == text.rstrip("\r\n").count("\n") + 1 and len(rows[-1][-1]) > 200
