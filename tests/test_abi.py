"""CPU: the C-ABI library loads and exports every symbol include/spfe.h declares;
host-side argument checking; weight-file round trip.  No compute calls."""
import ctypes
import os
import re

import numpy as np
import pytest

from sp_orb_slam_amd import extractor, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    declared = set(re.findall(r"SPFE_API[^;(]*?\b(spfe_\w+)\s*\(", hdr))
    assert declared == set(extractor.ABI_SYMBOLS)
    lib = ctypes.CDLL(extractor.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def _declarations():
    """name -> (return type, number of parameters) from the declarations of include/spfe.h; (void) and () count as 0."""
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    decls = {}
    for ret, name, params in re.findall(r"SPFE_API\s+([^;(]*?)\b(spfe_\w+)\s*\(([^;()]*)\)\s*;", hdr):
        params = params.strip()
        decls[name] = ("".join(ret.split()), 0 if params in ("", "void") else params.count(",") + 1)
    return decls


_RESTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "void": None,
             "void*": ctypes.c_void_p, "constchar*": ctypes.c_char_p}


def test_every_declared_symbol_is_bound_with_its_signature():
    """A call through ctypes without argtypes converts and checks nothing, and a wrong count fails only when the call is
    made: after load_library() every symbol the header declares has the restype of its declaration, and argtypes, as many
    as the declaration has parameters."""
    decls = _declarations()
    assert set(decls) == set(extractor.ABI_SYMBOLS)
    L = extractor.load_library()
    unbound = [name for name in sorted(decls)
               if getattr(L, name).argtypes is None or getattr(L, name).restype is not _RESTYPES[decls[name][0]]]
    assert not unbound, unbound
    miscounted = [(name, len(getattr(L, name).argtypes), n) for name, (_, n) in sorted(decls.items())
                  if len(getattr(L, name).argtypes) != n]
    assert not miscounted, miscounted


def test_abi_check_refuses_a_caller_built_against_another_header():
    """spfe_result / spfe_record_layout grew in round 3; a caller with the old strides must be refused up front."""
    import ctypes as C
    L = extractor.load_library()   # (itself calls spfe_check_abi with the ctypes mirrors' sizes)
    assert L.spfe_abi_version() == extractor.ABI_VERSION
    sizes = (C.sizeof(extractor._Config), C.sizeof(extractor._Result), C.sizeof(extractor.RecordLayout))
    assert L.spfe_check_abi(extractor.ABI_VERSION, *sizes) == 0
    assert L.spfe_check_abi(extractor.ABI_VERSION - 1, *sizes) == -1
    assert b"ABI" in L.spfe_last_error()
    assert L.spfe_check_abi(extractor.ABI_VERSION, sizes[0], sizes[1] - 8, sizes[2]) == -1   # round 2's spfe_result
    # the header and the Python mirror name the same revision
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    assert "#define SPFE_ABI_VERSION %d" % extractor.ABI_VERSION in hdr


def test_library_reports_version_and_stage_names():
    L = extractor.load_library()
    assert b"gfx950" in L.spfe_version()
    names = []
    while L.spfe_stage_name(len(names)):
        names.append(L.spfe_stage_name(len(names)).decode())
    assert names[0] == "conv1a" and names[-1] == "total" and "select" in names and "post_side" in names


def test_create_rejects_bad_config_without_gpu():
    blob = np.zeros(weights.NUM_PARAMS, np.float32)
    # size not a multiple of 8 is rejected before any HIP call (sp_extractor.cpp:70)
    with pytest.raises(extractor.SpfeError, match="multiples of 8"):
        extractor.SPExtractor(100, 100, 96, blob)
    with pytest.raises(extractor.SpfeError, match="num_features"):
        extractor.SPExtractor(0, 64, 96, blob)
    with pytest.raises(extractor.SpfeError, match="params"):
        extractor.SPExtractor(100, 64, 96, blob[:10])


def test_no_cpu_fallback():
    """Without a GPU the product must fail loudly, not compute on the host."""
    import subprocess
    import sys
    code = ("import numpy as np, sys; sys.path.insert(0, %r);"
            "from sp_orb_slam_amd import extractor, weights;"
            "from sp_orb_slam_amd.extractor import SPExtractor\n"
            "try:\n"
            "    SPExtractor(10, 64, 96, np.zeros(weights.NUM_PARAMS, np.float32)); print('CREATED')\n"
            "except extractor.SpfeError as e:\n"
            "    print('ERR', e)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env).stdout
    assert "CREATED" not in out and "SPFE_EHIP" in out


def test_weight_file_roundtrip(tmp_path):
    blob = weights.synthetic(3, "sparse")
    p = tmp_path / "w.spfw"
    weights.save(p, blob)
    assert np.array_equal(weights.load(p), blob)
    named = weights.to_named_tensors(blob)
    assert named["convPb.weight"].shape == (65, 256, 1, 1)
    assert np.array_equal(weights.from_named_tensors(named), blob)
    with open(p, "r+b") as f:
        f.write(b"XXXX")
    with pytest.raises(ValueError):
        weights.load(p)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under sp_orb_slam_amd/ or include/ may use it."""
    for base in ("sp_orb_slam_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for fn in files:
                if fn.endswith((".py", ".hip", ".cpp", ".h", ".hpp")):
                    txt = open(os.path.join(dirpath, fn), errors="ignore").read()
                    assert "oracle/" not in txt.replace("oracle/spfe_oracle.c);", "") or fn in ("spfe_exact_math.h", "spfe_dust_math.h"), fn  # headers shared with the oracle name it in a comment
                    assert "import oracle" not in txt and "from oracle" not in txt, fn


def _build_adaptor(tmpdir):
    import subprocess
    exe = os.path.join(str(tmpdir), "adaptor_main")
    pkg = os.path.join(ROOT, "sp_orb_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "stubs"),
                           os.path.join(ROOT, "tests", "cpp", "adaptor_main.cpp"), "-o", exe,
                           "-L" + pkg, "-lspfe", "-Wl,-rpath," + pkg])
    return exe


def _build_dropin(tmpdir):
    """tests/cpp/dropin_main.cpp: orbslam::SPExtractor (include/orbslam_sp_extractor.hpp) deriving
    BaseExtractor — the interface stand-in tests/stubs/orb_slam_iface."""
    import subprocess
    exe = os.path.join(str(tmpdir), "dropin_main")
    pkg = os.path.join(ROOT, "sp_orb_slam_amd")
    iface = os.path.join(ROOT, "tests", "stubs", "orb_slam_iface")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + iface,
                           os.path.join(ROOT, "tests", "cpp", "dropin_main.cpp"), "-o", exe,
                           "-L" + pkg, "-lspfe", "-Wl,-rpath," + pkg])
    return exe


def test_dropin_class_compiles_against_interface_stub(tmp_path):
    assert os.path.exists(_build_dropin(tmp_path))


def test_cpp_adaptor_compiles_and_links(tmp_path):
    """include/spfe_extractor.hpp (the BaseExtractor-shaped C++ host class) builds against the
    C ABI; OpenCV core is stood in for by tests/stubs (the image has no OpenCV)."""
    exe = _build_adaptor(tmp_path)
    assert os.path.exists(exe)
