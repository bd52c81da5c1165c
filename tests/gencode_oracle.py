"""The CPU oracle (oracle/rnacode_oracle.c) under another genetic code, for the tests of rc_params.genetic_code.

The oracle takes its code from one initialiser, GENETIC_CODE (codon index 16 n1 + 4 n2 + n3 with A=0 C=1 G=2 T=3), through g_pep /
pep_of; tests/test_oracle_golden.py pins it to the reference for the standard code.  variant(letters, tmpdir) compiles a copy with
that initialiser replaced, with the flags of oracle/Makefile's liboracle.so rule, and loads it through a second module instance of
oracle/binding.py, so that get_models, run_block, score_aln and backtrack work unchanged.  Nothing under oracle/ is written.
"""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = "-O2 -g -std=c99 -ffp-contract=off -fno-fast-math -fPIC -shared -Wall -Wextra".split()   # oracle/Makefile, liboracle.so
_TCAG = {"T": 0, "C": 1, "A": 2, "G": 3}


def internal_order(ncbi: str) -> str:
    """64 letters in NCBI's TCAG order -> the oracle's (and the library's) A, C, G, T order."""
    assert len(ncbi) == 64
    acgt = "ACGT"
    return "".join(ncbi[16 * _TCAG[acgt[c >> 4]] + 4 * _TCAG[acgt[(c >> 2) & 3]] + _TCAG[acgt[c & 3]]] for c in range(64))


def variant_source(internal: str) -> str:
    with open(os.path.join(ORACLE, "rnacode_oracle.c")) as fh:
        src = fh.read()
    pat = re.compile(r"static const char GENETIC_CODE\[\] =\s*(\"[^\"]*\"\s*)+;")
    hits = pat.findall(src)
    assert len(hits) == 1, "expected exactly one GENETIC_CODE initialiser in oracle/rnacode_oracle.c"
    lines = "\n".join('    "%s"' % internal[i:i + 16] for i in range(0, 64, 16))
    return pat.sub(lambda _m: "static const char GENETIC_CODE[] =\n" + lines + ";", src, count=1)


_CACHE = {}


def variant(ncbi: str, tmpdir):
    """A module instance of oracle/binding.py whose library scores with `ncbi` (64 letters, NCBI's TCAG order)."""
    if ncbi in _CACHE:
        return _CACHE[ncbi]
    internal = internal_order(ncbi)
    d = os.path.join(str(tmpdir), "oracle_" + str(len(_CACHE)))
    os.makedirs(d, exist_ok=True)
    src = os.path.join(d, "rnacode_oracle.c")
    with open(src, "w") as fh:
        fh.write(variant_source(internal))
    so = os.path.join(d, "liboracle.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), *CFLAGS, "-I", ORACLE, "-o", so, src, "-lm"])
    name = "oracle_binding_gencode_" + str(len(_CACHE))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ORACLE, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod   # (its dataclasses look their module up there)
    spec.loader.exec_module(mod)
    mod._LIB_PATH = so
    mod.build = lambda force=False: so   # never remake the stock library from here
    _CACHE[ncbi] = mod
    return mod
