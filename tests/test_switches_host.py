"""The switch table of DESIGN.md §9 against the code (no GPU): every ``STV_*`` environment variable the
package reads has a row, every row names a variable the package reads, and the switches whose losing
arm was removed (``profiles/patches/step_variants_removed.patch``) are gone from code, tools and tests.
"""
from __future__ import annotations

import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "style_transfer_visualizer_amd"

REMOVED = ("STV_SIDE_LANE", "STV_LBFGS_PIPE", "STV_LBFGS_NT", "STV_LBFGS_ACC", "STV_GRAM_FIN_MERGE", "STV_GRAM_MERGE")

_C_READ = re.compile(r'getenv\("(STV_[A-Z0-9_]+)"\)')
_PY_READ = re.compile(r'os\.environ(?:\.get\(|\.setdefault\(|\[)\s*["\'](STV_[A-Z0-9_]+)["\']')


def _names_read_by_the_package() -> set[str]:
    names: set[str] = set()
    for path in sorted((PKG / "csrc").iterdir()):
        if path.suffix in (".hip", ".h"):
            names.update(_C_READ.findall(path.read_text()))
    for path in sorted(PKG.rglob("*.py")):
        names.update(_PY_READ.findall(path.read_text()))
    return names


def _names_in_the_design_table() -> set[str]:
    text = (ROOT / "DESIGN.md").read_text()
    section = text[text.index("## 9. Environment switches"):]
    names: set[str] = set()
    for line in section.splitlines():
        if line.startswith("| `STV_"):
            names.update(re.findall(r"STV_[A-Z0-9_]+", line.split("|")[1]))
    return names


def test_design_switch_table_matches_the_variables_the_package_reads():
    code, table = _names_read_by_the_package(), _names_in_the_design_table()
    assert code - table == set(), "read by the package, no row in DESIGN.md §9"
    assert table - code == set(), "row in DESIGN.md §9, read nowhere in the package"
    assert len(code) == len(table) == 36


def test_removed_switches_are_named_nowhere_in_code_tools_or_tests():
    pattern = re.compile(r"(?<![A-Z0-9_])(?:" + "|".join(REMOVED) + r")(?![A-Z0-9_])")
    hits = []
    for top in (PKG, ROOT / "tools", ROOT / "tests"):
        for path in sorted(top.rglob("*")):
            if not path.is_file() or "__pycache__" in path.parts or path == Path(__file__).resolve():
                continue
            try:
                text = path.read_text(encoding="utf-8")
            except UnicodeDecodeError:      # build products, golden vectors
                continue
            hits += [f"{path.relative_to(ROOT)}: {m.group(0)}" for m in pattern.finditer(text)]
    assert hits == []
