"""CPU: README's table of environment switches and the $PSK_* switches the library reads are the same set."""
import os
import re

from conftest import ROOT

NAME = r'"(PSK_[A-Z0-9_]+)"'


def _files(top, exts):
    for d, _, names in os.walk(top):
        for n in names:
            if n.endswith(exts):
                yield os.path.join(d, n)


def _read_by_library():
    """Names that pyskani_amd/ hands to getenv (env_val wraps it), os.environ or the PSK_SWITCHES X-macro."""
    found = set()
    for path in _files(os.path.join(ROOT, "pyskani_amd"), (".hip", ".h", ".c", ".cpp", ".py")):
        text = open(path).read()
        found |= set(re.findall(r"\b(?:getenv|env_val)\(\s*" + NAME, text))
        found |= set(re.findall(r"\bos\.environ(?:\.get\(|\[)\s*" + NAME, text))
        found |= set(re.findall(r"\bX\(\w+,\s*" + NAME + r"\)", text))
    return found


def _used_by_tests():
    found = set()
    for path in _files(os.path.join(ROOT, "tests"), (".py",)):
        if os.path.basename(path) == os.path.basename(__file__):
            continue
        text = open(path).read()
        found |= set(re.findall(NAME, text)) | set(re.findall(r"\b(PSK_[A-Z0-9_]+)=", text))
    return found


def _readme_table():
    text = open(os.path.join(ROOT, "README.md")).read()
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("| `PSK_")]
    return set(re.findall(r"\bPSK_[A-Z0-9_]+", "\n".join(rows)))


def test_every_switch_the_library_reads_is_in_the_readme_table():
    read = _read_by_library()
    assert len(read) >= 40, sorted(read)      # (the scan itself still finds the switches)
    missing = read - _readme_table()
    assert not missing, sorted(missing)


def test_every_switch_in_the_readme_table_is_still_read():
    stale = _readme_table() - _read_by_library() - _used_by_tests()
    assert not stale, sorted(stale)
