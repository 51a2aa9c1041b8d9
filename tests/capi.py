"""What the host tests of the C ABI share: the header without its comments, the library's export set and the check of
a refusal.  No torch, no oracle."""
import functools
import re
import subprocess

from spconv_amd import _lib

with open(_lib.HEADER_PATH) as _f:
    HEADER = re.sub(r"/\*.*?\*/", "", _f.read(), flags=re.S)


def declared():
    """every spx_ name the header puts before a `(`"""
    return sorted(set(re.findall(r"\b(spx_[a-z0-9_]+)\s*\(", HEADER)))


@functools.lru_cache(maxsize=None)
def exported():
    """the symbols libspconv_amd.so defines (nm runs once per session)"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    return frozenset(line.split()[-1] for line in out.splitlines() if " T " in line)


def fails(rc, word):
    assert rc != 0
    assert word in _lib.load().spx_last_error().decode(), _lib.load().spx_last_error()
