"""The environment variables the product reads are exactly the ones
INTEGRATION.md documents, and no compile-time experiment block is left in the
kernels (a text scan: no build, no GPU)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "bulletproof-perm_amd"


def csrc_files():
    return [p for p in sorted((PKG / "csrc").rglob("*")) if p.is_file()]


def read_by_code():
    names = set()
    for p in csrc_files():
        names |= set(re.findall(r'getenv\(\s*"(BPP_[A-Z0-9_]+)"', p.read_text()))
    for p in sorted((PKG / "bpperm").glob("*.py")) + [PKG / "build.py"]:
        names |= set(re.findall(r'environ(?:\.get\(|\.setdefault\(|\[)\s*["\'](BPP_[A-Z0-9_]+)["\']', p.read_text()))
    return names


def documented():
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"^### Environment variables\n(.*?)(?=^#{2,3} )", text, flags=re.M | re.S)
    assert m, "INTEGRATION.md has no 'Environment variables' section"
    return set(re.findall(r"^\| `(BPP_[A-Z0-9_]+)` \|", m.group(1), flags=re.M))


def test_documented_variables_are_the_ones_read():
    code, doc = read_by_code(), documented()
    assert code, "the scan found no variable at all"
    assert code == doc, {"read but not documented": sorted(code - doc), "documented but not read": sorted(doc - code)}


def test_no_experiment_blocks_in_csrc():
    hits = [f"{p.relative_to(ROOT)}: {m}" for p in csrc_files() for m in re.findall(r"\bEXP_[A-Z0-9_]+", p.read_text())]
    assert not hits, hits
