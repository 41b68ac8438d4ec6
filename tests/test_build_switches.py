"""The compile-time switches of the native sources and their table in DESIGN.md section 3 ("Build switches") stay
equal (CPU, text only: nothing is compiled).

- every `WCPT_*` name that a preprocessor condition (`#if` / `#ifdef` / `#ifndef` / `#elif`, `defined()` included) under
  wc-path-tracer_amd/csrc or wc-path-tracer_amd/host tests has a row in the table, and every row is still tested
  somewhere. Include guards (`*_H`) and the names include/wcpt.h defines (the ABI's constants) are no switches;
- every `-DWCPT_*` that a file under tools/ names has a row. The shell scripts of single past rounds (`_r0N` in the
  file name) are history and exempt.

An experiment that adds a switch so documents it, and one that ends either keeps the switch with its row or removes
both.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wc-path-tracer_amd")
NAME = re.compile(r"\bWCPT_[A-Z0-9_]+\b")
CONDITION = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top):
    for d, _, names in sorted(os.walk(top)):
        for n in sorted(names):
            yield os.path.join(d, n)


def conditional_names(text):
    """WCPT_* names in the conditions of `text`'s preprocessor conditionals (continuation lines joined)."""
    out = set()
    for cond in CONDITION.findall(text.replace("\\\n", " ")):
        out.update(NAME.findall(cond))
    return out


def table_names(design):
    section = design.split("### Build switches", 1)[1]
    section = re.split(r"^#{2,3} ", section, maxsplit=1, flags=re.M)[0]
    rows = re.findall(r"^\| `(WCPT_[A-Z0-9_]+)` \|", section, re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows"
    return set(rows)


def source_switches():
    abi = set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(WCPT_[A-Z0-9_]+)", _read(os.path.join(ROOT, "include", "wcpt.h")), re.M))
    names = set()
    for sub in ("csrc", "host"):
        for path in _files(os.path.join(PKG, sub)):
            names |= conditional_names(_read(path))
    return {n for n in names if not n.endswith("_H")} - abi


def test_parser_sees_every_conditional_form():
    text = ("#if WCPT_A && defined(__gfx9__)\n#elif defined(WCPT_B) || \\\n    !defined( WCPT_C )\n#endif\n"
            "  # ifdef WCPT_D\n#ifndef WCPT_E_H\n#define WCPT_F 1\nint x = WCPT_G;\n")
    assert conditional_names(text) == {"WCPT_A", "WCPT_B", "WCPT_C", "WCPT_D", "WCPT_E_H"}


def test_sources_and_table_name_the_same_switches():
    table = table_names(_read(os.path.join(ROOT, "DESIGN.md")))
    src = source_switches()
    assert src - table == set(), "tested in the sources without a row in DESIGN.md's Build switches table"
    assert table - src == set(), "rows of DESIGN.md's Build switches table that no source tests"


def test_tools_define_only_documented_switches():
    table = table_names(_read(os.path.join(ROOT, "DESIGN.md")))
    stray = {}
    for path in _files(os.path.join(ROOT, "tools")):
        if re.search(r"_r0\d", os.path.basename(path)):
            continue
        used = set(re.findall(r"-D(WCPT_[A-Z0-9_]+)", _read(path))) - table
        if used:
            stray[os.path.relpath(path, ROOT)] = sorted(used)
    assert stray == {}
