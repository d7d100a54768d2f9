"""regexp_replace(str, pattern, replacement, 'g') on the host (comet_regexp_replace_host: csrc/regex.cpp compile_regex_replace + the SAME source the
kernels run, csrc/device/regex_vm.hpp rx_replace): the reference's own vectors (sql-tests/expressions/string/regexp_replace_rust.sql), find_iter's rule for
empty matches, the crate's Captures::expand rules for the replacement, every refusal by name, and generated patterns against the oracle's restatement of
the iteration (oracle.find_iter_like_the_crate)."""
import os
import random
import re
import sys

import pytest

from datafusion_comet_amd import native, serde as S
from tests.test_regexp_extract_cpu import ALPHA, gen

rr = native.regexp_replace_host
STR, I32 = S.T_STRING, S.T_INT32


def test_reference_vectors():
    assert [rr(r"(\d+)", "X", v) for v in ("100-200", "abc", "", "phone 123-456-7890")] == ["X-X", "abc", "", "phone X-X-X"]


def test_empty_matches_follow_find_iter():
    assert rr("x*", "-", "axxbéc") == "-a-b-é-c-"      # (advancing by a byte would cut é in two)
    assert rr("a*", "-", "baac") == "-b-c-"            # (Python's re.sub: '-b--c-' — the empty match behind 'aa' is dropped)
    assert rr("", "-", "abc") == "-a-b-c-"
    assert rr("", "-", "") == "-"
    assert rr(r"\b", "|", "ab cd") == "|ab| |cd|"
    assert rr(r"(?m)^", "> ", "a\nb\n") == "> a\n> b\n> "


def test_replacement_template():
    assert rr(r"(\w+)@(\w+)", "${2} at $1 $$", "joe@example, bob@site") == "example at joe $, site at bob $"
    assert rr("(a)|b", "[$1]", "ab") == "[a][]"                     # a group that took no part expands to nothing
    assert rr(r"\d+", "<$0>", "a12b3") == "a<12>b<3>"
    assert rr(r"\d+", "$0$", "a12b") == "a12$b"                     # a trailing $ is itself
    assert rr(r"\d+", "${", "a12b") == "a${b" and rr(r"\d+", "${1", "a12b") == "a${1b"      # ${ without } likewise
    assert rr(r"\d+", "$-$ ", "a1b") == "a$-$ b"
    assert rr(r"(\d)(\d)", "$2$1$2", "12 34") == "212 434"
    assert rr(r"(\d)", "${1}0", "a1") == "a10" and rr(r"(é+)", "«$1»", "cafééé!") == "caf«ééé»!"
    assert rr("(a)(b)(c)(d)", "$4$3$2$1$0", "abcd") == "dcbaabcd"   # four distinct groups ≥ 1 and group 0
    assert rr("b", "", "abcb") == "ac" and rr("z", "y", "abc") == "abc"


def test_refusals_name_the_construct():
    for pat, rep, why in ((r"(a)", "$1a", r"'\$1a' names a group"), (r"(a)", "${name}", r"'\$\{name\}' names a group"), (r"(a)", "${}", "names a group"),
                          (r"(a)", "$2", r"in `regexp_replace` is invalid: Expects group index between 0 and 1, but got 2"), (r"a", "$1", r"between 0 and 0, but got 1"),
                          (r"(a)", "$12345678901", "Expects group index between 0 and 1"), (r"(a)", r"\1", "backslash"), (r"(a)", r"x\\y", "backslash"),
                          (r"(a)(b)(c)(d)(e)", "$1$2$3$4$5", "more than 4 distinct groups"), (r"\p{L}", "x", "not supported"), (r"(?P<n>a)", "x", "named groups"),
                          (r"(a*)*", "x", "empty string"), (r"(unclosed", "x", "unclosed group")):
        with pytest.raises(native.CometNativeException, match=why):
            rr(pat, rep, "abc")


def _plan_error(expr):
    ok, msg = native.check_plan(S.project(S.scan([STR, I32]), [expr]).encode())
    assert not ok
    return msg


def test_refusals_at_create_plan(built):
    s, L = S.col(0, STR), lambda v: S.lit(v, STR)
    f = lambda args: S.scalar_func("regexp_replace", args, STR)      # noqa: E731
    assert "Utf8 COLUMN" in _plan_error(S.regexp_replace(S.scalar_func("upper", [s], STR), "a", "b"))
    assert "NULL pattern" in _plan_error(f([s, L(None), L("x"), L("g")])) and "NULL replacement" in _plan_error(f([s, L("a"), L(None), L("g")]))
    assert "pattern must be a string literal" in _plan_error(f([s, s, L("x"), L("g")])) and "replacement must be a string literal" in _plan_error(f([s, L("a"), s, L("g")]))
    assert "flags argument must be the literal 'g'" in _plan_error(f([s, L("a"), L("x"), L("i")])) and "literal 'g'" in _plan_error(f([s, L("a"), L("x"), s]))
    assert "expects 4 arguments" in _plan_error(f([s, L("a"), L("x")]))
    assert "backslash" in _plan_error(S.regexp_replace(s, "(a)", r"\1")) and "between 0 and 1, but got 2" in _plan_error(S.regexp_replace(s, "(a)", "$2"))
    assert "not supported" in _plan_error(S.regexp_replace(s, r"\p{L}", "x")) and "names a group" in _plan_error(S.regexp_replace(s, "(a)", "$1a"))
    assert "more than 4 distinct groups" in _plan_error(S.regexp_replace(s, "(a)(b)(c)(d)(e)", "$1$2$3$4$5"))


def expected(rx, segments, text):
    """the rule itself over the oracle's find_iter: the text between the matches, the template (str | group number) per match, the rest"""
    from oracle import oracle as O
    out, last = [], 0
    for m in O.find_iter_like_the_crate(rx, text):
        out.append(text[last:m.start()])
        out.extend(seg if isinstance(seg, str) else (m.group(seg) or "") for seg in segments)
        last = m.end()
    return "".join(out) + text[last:]


def test_against_the_oracles_restatement():
    from oracle import oracle as O
    rng = random.Random(79)
    checked = with_group = 0
    for _ in range(500):
        groups = [0]
        pat = gen(rng, 2, groups)
        try:
            rx = O.crate_pattern_to_python(pat)
        except re.error:
            continue
        for _ in range(4):
            text = "".join(rng.choice(ALPHA) for _ in range(rng.randint(0, 10)))
            idx = rng.randint(0, groups[0])
            try:
                got = rr(pat, "<${%d}>" % idx, text)
            except Exception as e:  # noqa: BLE001
                assert "not supported" in str(e), (pat, str(e))
                break
            assert got == expected(rx, ["<", idx, ">"], text), (pat, idx, text)
            checked += 1
            with_group += idx >= 1
    assert checked >= 1500 and with_group >= 200, (checked, with_group)


def test_plans_pass_check_plan_and_compile(built):
    s = S.col(0, STR)
    strip = S.regexp_replace(s, "[^0-9]", "")
    proj = S.project(S.scan([STR, I32]), [strip, S.regexp_replace(s, r"(\w+)@(\w+)", "${2} at $1"), strip, S.scalar_func("length", [strip], I32), S.col(1, I32)])
    filt = S.project(S.filter_(S.scan([STR, I32]), S.eq(S.regexp_replace(s, "-", ""), S.lit("100200", STR))), [s])
    for plan in (proj, filt):
        ok, msg = native.check_plan(plan.encode())
        assert ok, msg
        assert native.compile_plan(plan.encode())
    # the same expression twice shares one derived column: three expressions, two columns computed over the source
    assert native.plan_codegen(proj.encode(), [True, False])["derived"] == 2


def test_the_sheet_no_longer_disables_it(built):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import compat_sheet as C
    text = C.render()
    assert "RegExpReplace" in C.probes() and "spark.comet.expression.RegExpReplace.enabled=false" not in text and "| `RegExpReplace` |" in text
