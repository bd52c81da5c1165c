"""rc_params.genetic_code on the host (no GPU): the built-in NCBI tables, the checks both drivers make while parsing options, the
oracle variant the GPU tests compare against (tests/gencode_oracle.py), and the resources of the two preparation kernels that read
the code at run time."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gencode_oracle as go
from conftest import ROOT, hss_key, load_golden
from helpers import block_from_golden
from oracle import binding as ob
from rnacode_amd import api

NCBI = {
    1: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    2: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG",
    3: "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    4: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    5: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG",
    6: "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    9: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    10: "FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    11: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    12: "FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    13: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG",
    14: "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    16: "FFLLSSSSYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    21: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    22: "FFLLSS*SYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    23: "FF*LSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    24: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG",
    25: "FFLLSSSSYY**CCGWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    26: "FFLLSSSSYY**CC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    29: "FFLLSSSSYYYYCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    30: "FFLLSSSSYYEECC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    33: "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG",
}
K_GENETIC_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"   # rc_tables.h, A C G T order
BAD_CODES = {
    "63 letters": NCBI[2][:63],
    "B": "B" + NCBI[2][1:],
    "X": NCBI[2][:10] + "X" + NCBI[2][11:],
    "lower case": NCBI[2].lower(),
    "all stops": "*" * 64,
}


def test_builtin_tables_match_ncbi():
    for i, letters in NCBI.items():
        assert api.genetic_code(i) == letters, i
    assert go.internal_order(api.genetic_code(1)) == K_GENETIC_CODE
    with open(os.path.join(ROOT, "rnacode_amd", "csrc", "rc_tables.h")) as fh:
        src = fh.read()
    m = re.search(r"kGeneticCode\[\] =\s*((?:\"[^\"]*\"\s*)+);", src)
    assert "".join(re.findall(r"\"([^\"]*)\"", m.group(1))) == K_GENETIC_CODE


@pytest.mark.parametrize("bad_id", [0, -1, 7, 8, 15, 17, 18, 19, 20, 27, 28, 31, 32, 34, 1000])
def test_unknown_ids_are_rejected(bad_id):
    with pytest.raises(api.RnacodeError) as ei:
        api.genetic_code(bad_id)
    assert ei.value.code == api.RC_ERR_ARG


def test_code_tables_follow_the_code():
    pep1, mat1 = api.code_tables(62)
    for same in (1, 11, "", NCBI[1]):
        pep, mat = api.code_tables(62, same)
        np.testing.assert_array_equal(pep, pep1)
        np.testing.assert_array_equal(mat, mat1)
    order = "ARNDCQEGHILKMFPSTWYV"
    for i, letters in NCBI.items():
        pep, _ = api.code_tables(90, i)
        internal = go.internal_order(letters)
        assert [(-1 if ch == "*" else order.index(ch)) for ch in internal] == pep.tolist(), i
    # vertebrate mitochondrial: TGA (codon 16*3 + 4*2 + 0) is Trp, AGA / AGG stops
    pep2, _ = api.code_tables(62, 2)
    assert pep2[56] == order.index("W") and pep1[56] == -1
    assert pep2[8] == -1 and pep2[10] == -1 and pep1[8] == order.index("R")
    assert api.default_params(genetic_code=2).genetic_code.decode() == NCBI[2]
    assert api.default_params(genetic_code="2").genetic_code.decode() == NCBI[2]
    assert api.default_params().genetic_code == b""


def test_details_codon_classes_follow_the_code():
    """--details classifies an in-frame codon pair with the run's own tables: TGA / TGG are both Trp under table 2, where AGA is a stop."""
    from rnacode_amd import details
    mito, standard = api.code_tables(62, 2), api.code_tables(62)
    assert details.codon_kind("TGA", "TGG", *mito) == "synonymous" and details.codon_kind("TGG", "TGA", *mito) == "synonymous"
    assert details.codon_kind("TGA", "TGA", *mito) == "identical"
    assert details.codon_kind("AGA", "AGA", *mito) == "stop" and details.codon_kind("CGT", "AGA", *mito) == "stop"
    assert details.codon_kind("TGA", "TGG", *standard) == "stop" and details.codon_kind("TGA", "TGA", *standard) == "stop"
    assert details.codon_kind("AGA", "AGA", *standard) == "identical" and details.codon_kind("CGT", "AGA", *standard) == "synonymous"
    assert details.codon_kind("AGA", "AAA", *standard) == "conservative"   # Arg / Lys: BLOSUM62 +2


@pytest.mark.parametrize("what", sorted(BAD_CODES))
def test_bad_codes_are_rejected_on_the_host(what):
    with pytest.raises(api.RnacodeError) as ei:
        api.default_params(genetic_code=BAD_CODES[what])
    assert ei.value.code == api.RC_ERR_ARG
    with pytest.raises(api.RnacodeError):
        api.code_tables(62, BAD_CODES[what])
    with pytest.raises(api.RnacodeError):   # 65 letters do not fit rc_params
        api.default_params(genetic_code=NCBI[2] + "A")


def _driver_argvs(code):
    native = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    inp = os.devnull   # never read: the option is refused first
    return [[native, "--genetic-code", code, inp], [sys.executable, "-m", "rnacode_amd.cli", "--genetic-code", code, inp]]


@pytest.mark.parametrize("code", ["7", "27", "0", BAD_CODES["63 letters"], BAD_CODES["lower case"], BAD_CODES["all stops"], BAD_CODES["B"]])
def test_drivers_reject_bad_codes_while_parsing(code):
    if not os.path.exists(os.path.join(ROOT, "rnacode_amd", "rnacode_hip")):
        api.build_library()
    env = dict(os.environ, RC_TRACE="1")
    for argv in _driver_argvs(code):
        r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0, argv
        assert "--genetic-code" in r.stderr, r.stderr
        assert "HIP device" not in r.stderr and "ctx:" not in r.stderr, r.stderr   # failed before any context was asked for
        assert r.stdout == "", r.stdout


def test_help_shows_the_option():
    for argv in _driver_argvs("1"):
        r = subprocess.run(argv[:1] + (["-m", "rnacode_amd.cli"] if argv[0] == sys.executable else []) + ["--help"], cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert "--genetic-code" in r.stdout + r.stderr


def _run(mod, entry, n=24, seed=7):
    b = block_from_golden(entry)
    ref = entry["ref"]
    return mod.run_block([r.seq for r in b.rows], [r.name for r in b.rows], b.rows[0].start, b.rows[0].length, ref["tree"], ref["kappa"],
                         mod.default_params(n), seed)


def _scored(doc):
    return [e for e in doc["blocks"] if "skipped" not in e["ref"]]


def test_oracle_variant_of_the_standard_code_is_the_stock_oracle(tmp_path):
    v1 = go.variant(NCBI[1], tmp_path)
    assert v1 is not ob and v1._LIB_PATH != ob._LIB_PATH
    for name in ("coding_maf_n100", "edge_cases_n50", "synth_6x120_n200"):
        for e in _scored(load_golden(name))[:3]:
            got, want = _run(v1, e), _run(ob, e)
            for g, w in zip(got.models + got.modelsRev, want.models + want.modelsRev):
                np.testing.assert_array_equal(np.float32(g["scores"]), np.float32(w["scores"]))
                np.testing.assert_array_equal(np.float32(g["probs"]), np.float32(w["probs"]))
            assert sorted(got.hss, key=hss_key) == sorted(want.hss, key=hss_key)
            np.testing.assert_array_equal(np.float32(got.maxScores), np.float32(want.maxScores))


def test_oracle_variant_of_a_ciliate_code_scores_taa_as_gln(tmp_path):
    """Table 6 reads TAA and TAG as Gln: on a block whose reference row has an in-frame TAA, the HSS list changes."""
    v6 = go.variant(NCBI[6], tmp_path)
    tried = differ = 0
    for e in _scored(load_golden("genomic_preprocessed_n100")):
        ref_row = block_from_golden(e).rows[0].seq.replace("-", "")
        if "TAA" not in ref_row:   # (in frame i % 3 of either strand's reading: every frame is scored)
            continue
        got, want = _run(v6, e, n=8), _run(ob, e, n=8)
        tried += 1
        differ += sorted(got.hss, key=hss_key) != sorted(want.hss, key=hss_key)
        if tried == 6:
            break
    assert tried > 0 and differ > 0, (tried, differ)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_run_time_code_kernels_use_no_lds_and_no_scratch(tmp_path):
    """They run beside k_null, whose workgroups hold all of a CU's LDS."""
    out = str(tmp_path / "rc_kernels.s")
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", *flags, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "rnacode_amd", "csrc", "rc_kernels.hip"), "-o", out])
    with open(out) as fh:
        txt = fh.read()
    for name in ("_ZN2rc16k_prep_models_rtENS_8PrepArgsE", "_ZN2rc20k_prep_models_few_rtENS_8PrepArgsE"):
        head = txt[txt.index(".amdhsa_kernel " + name + "\n"):]
        head = head[:head.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", head).group(1)) == 0, name


class _ParamsV1(ctypes.Structure):
    """rc_params as programs compiled against the header of before genetic_code know it (40 bytes)."""
    _fields_ = [("Delta", ctypes.c_float), ("Omega", ctypes.c_float), ("omega", ctypes.c_float), ("stopPenalty_0", ctypes.c_float),
                ("stopPenalty_k", ctypes.c_float), ("blosum", ctypes.c_int32), ("sampleN", ctypes.c_int32), ("cutoff", ctypes.c_float),
                ("stopEarly", ctypes.c_int32), ("seed_base", ctypes.c_uint32)]


def test_older_layout_callers_keep_their_entry_points():
    """A binary built against the older header calls rc_default_params with a 40-byte struct: nothing past it may be written.  The
    header maps the names to the _v2 entry points, which fill the whole struct."""
    assert ctypes.sizeof(_ParamsV1) == 40 == api.RcParams.genetic_code.offset
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    for name in api.COMPAT_SYMBOLS:
        assert re.search(r"#define %s %s_v2\b" % (name, name), hdr), name
        assert hasattr(api.lib(), name), name

    class Guarded(ctypes.Structure):
        _fields_ = [("p", _ParamsV1), ("canary", ctypes.c_uint8 * 96)]

    g = Guarded()
    ctypes.memset(ctypes.addressof(g.canary), 0xA5, 96)
    api.lib().rc_default_params(ctypes.byref(g.p))
    assert bytes(g.canary) == b"\xa5" * 96
    want = api.default_params()
    for name, _ in _ParamsV1._fields_:
        assert getattr(g.p, name) == getattr(want, name), name
    full = api.RcParams()
    ctypes.memset(ctypes.byref(full), 0x41, ctypes.sizeof(full))
    api.lib().rc_default_params_v2(ctypes.byref(full))
    assert full.genetic_code == b""
