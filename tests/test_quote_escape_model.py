"""The escape-aware part of the lane model (tools/emulate_quote.py) against the definition, the byte loop of
tests/_escape_loop.py: escape runs across every chunk, row, wave and tile edge, an all-escape tile, esc_carry at every
alignment, the u16b form entered deep in its block, random bytes across more than 130 tiles under the look-back
schedules, the walk-back bound, and the deliberate defects of emu.ESCAPE_MUTANTS, each noticed by these cases."""
import csv as pycsv
import io
import itertools
import os
import sys

import numpy as np
import pytest

import _escape_cases as C
from _escape_loop import loop_record_ends

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emulate_quote as emu  # noqa: E402

T = emu.TILE_BYTES


def test_constants_mirror_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpquote.h")).read()
    from dataplug_amd.scan import _quote
    assert "#define DQ_ESCAPE_RUN_MAX (1u << 20)" in text and "#define DQ_ERR_ESCAPE_RUN 6" in text
    assert emu.ESCAPE_RUN_MAX == _quote.DQ_ESCAPE_RUN_MAX == 1 << 20 >= T + 16
    assert _quote.DQ_ERR_ESCAPE_RUN == 6 and _quote.DQ_ESC_SCOPE_QUOTED == emu.ESC_SCOPE_QUOTED == 1


def test_loop_cuts_writer_output_where_csv_reader_does():
    """Objects written by csv.writer(escapechar='\\\\', doublequote=False): every piece between the loop's record ends
    (scope "all") parses back to exactly one row, the row of the whole-object parse."""
    dialect = dict(quotechar='"', escapechar="\\", doublequote=False, lineterminator="\n")
    alphabet = 'ab,"\\\n x'
    n = 0
    for quoting in (pycsv.QUOTE_MINIMAL, pycsv.QUOTE_ALL, pycsv.QUOTE_NONE):
        fields = ["".join(t) for k in (0, 1, 2) for t in itertools.product(alphabet, repeat=k)]
        rng = np.random.default_rng(quoting)
        for _ in range(600):
            rows = [[fields[i] for i in rng.integers(0, len(fields), int(rng.integers(1, 4)))]
                    for _ in range(int(rng.integers(1, 5)))]
            rows = [r for r in rows if r != [""]] or [["a"]]         # (a lone empty field is written as a bare line)
            s = io.StringIO()
            pycsv.writer(s, quoting=quoting, **dialect).writerows(rows)
            text = s.getvalue()
            whole = list(pycsv.reader(io.StringIO(text, newline=""), quoting=quoting, **dialect))
            ends = loop_record_ends(np.frombuffer(text.encode(), np.uint8), scope="all")[0]
            assert len(ends) == len(whole) and (len(text) == 0 or int(ends[-1]) == len(text) - 1), text
            lo = 0
            for e, row in zip(ends, whole):
                piece = list(pycsv.reader(io.StringIO(text[lo:int(e) + 1], newline=""), quoting=quoting, **dialect))
                assert piece == [row], (text, lo, int(e))
                lo = int(e) + 1
            n += 1
    assert n == 1800


def test_esc_code_is_the_loop_on_every_chunk():
    e = np.arange(1 << 16)
    for inb in (0, 1):
        c = emu.esc_code(e, inb)
        escaped, out = (c ^ (e | inb)) & 0xFFFF, ((c & e) >> 15) & 1
        for m in range(0, 1 << 16, 97):                  # the loop on a sample, the closed form on all
            esc, want = inb, 0
            for i in range(16):
                if esc:
                    want |= 1 << i
                    esc = 0
                elif (m >> i) & 1:
                    esc = 1
            assert (int(escaped[m]), int(out[m])) == (want, esc), (m, inb)


@pytest.mark.parametrize("edges", [C.EDGES_ODD, C.EDGES_EVEN], ids=["odd", "even"])
def test_runs_ending_at_every_edge(edges):
    for c in C.edge_cases(edges):
        C.check_model(emu, c, forms=("u64",) if len(c["name"]) % 2 else ("u32", "u16b"))


def test_exact_runs_and_one_more():
    for c in C.exact_run_cases():
        C.check_model(emu, c, forms=("u64", "u16b"))


def test_all_escape_tile_between_two_ordinary_ones():
    for c in C.all_escape_tile_cases():
        for sched in ("sequential", "all_agg"):
            C.check_model(emu, c, schedule=sched)


def test_begin_at_every_alignment_carry_esc_carry_scope():
    cases = C.alignment_cases()
    assert len(cases) == 16 * 8
    for c in cases:
        C.check_model(emu, c)


def test_blocked_form_entered_deep_in_its_block():
    for c in C.blocked_large_begin_cases():
        assert c["begin"] & 0xFFFF >= 40000
        C.check_model(emu, c)


def test_random_bytes_across_130_tiles_under_the_schedules():
    d = C.random_five(131 * T + 333, 2024)
    c = C.case(d, begin=3, carry=1, esc_carry=1, scope="all")
    exp = C.expect(c)
    assert emu.host_args(0, len(d), 0, 3, len(d)).ntiles >= 130
    for sched in ("sequential", "all_agg", "chain_to_tile0", "window_edge", "random:5"):
        C.check_model(emu, c, exp, forms=("u64",), schedule=sched)
    C.check_model(emu, c, exp, forms=("u16b",), schedule="random:2")
    cq = dict(c, scope="quoted", carry=0)
    C.check_model(emu, cq, forms=("u64",), schedule="random:1")


def killers():
    return C.all_escape_tile_cases() + C.alignment_cases()[:32] + C.exact_run_cases()[:4] + \
        [C.case(C.random_five(T + 50, 3), esc_carry=1)]


@pytest.mark.parametrize("mutant", emu.ESCAPE_MUTANTS)
def test_each_escape_mutant_is_killed(mutant):
    killed = 0
    for c in killers():
        ends, nq, nn, tog = C.expect(c)
        r = C.model(emu, c, "u64", mutate=mutant)
        ok = np.array_equal(r[0], ends) and r[-5:] == (len(ends), nq, nn, 0, tog)
        killed += not ok
    assert killed > 0, f"no case notices the defect {mutant}"


def test_escape_mutants_change_nothing_without_an_escape():
    d = C.random_five(T + 77, 8)
    want = emu.run(d, begin=5, carry=1)
    for mutant in emu.ESCAPE_MUTANTS:
        got = emu.run(d, begin=5, carry=1, mutate=mutant)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
    assert "all_escape_resets" not in emu.MUTANTS + emu.BLOCKED_MUTANTS


def test_an_absent_escape_byte_changes_nothing():
    d = C.random_five(2 * T + 9, 4)
    for fmt, u64 in ((None, True), (None, False), ("u16b", True)):
        want = emu.run(d, begin=0, carry=1, u64=u64, fmt=fmt)
        got = emu.run(d, begin=0, carry=1, u64=u64, fmt=fmt, escape=7, esc_carry=0)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))


def test_a_run_up_to_the_bound_is_exact_and_one_chunk_more_is_the_error():
    n0 = 16384                                           # the run ends at a wave's first byte, chunk-aligned
    for extra, err in ((0, 0), (16, emu.ERR_ESCAPE_RUN)):
        L = emu.ESCAPE_RUN_MAX + extra
        d = C.plain(n0 + L + 40, 1)
        d[n0 - 1 - extra] = ord("a")
        d[n0 - extra:n0 - extra + L] = C.E
        C.after_run(d, n0 - extra + L)
        c = C.case(d)
        r = C.model(emu, c)
        assert r[-2] == err
        if not err:
            C.check_model(emu, c, forms=("u64",))


def test_model_refuses_what_the_entry_points_refuse():
    d = C.random_five(100, 1)
    for kw in (dict(escape=34), dict(escape=10), dict(escape=256), dict(escape=92, esc_carry=2),
               dict(escape=92, escape_scope="some")):
        with pytest.raises(ValueError):
            emu.run(d, **kw)
