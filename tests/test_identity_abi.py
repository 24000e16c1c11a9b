"""CPU checks of the identity-column boundary (include/fseq.h, fseq_identity_columns .. fseq_write_founders_restored): the
symbols, the struct layout, the refusals that must not touch a device, the front end's options -- and the numpy model the
GPU tests (tests/test_gpu_identity.py) lean on, pinned to the built host tools remove_identity_columns and
insert_identity_columns, which are the yardstick."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import identity_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fseq_identity_columns", "fseq_create_without_identity_columns", "fseq_get_identity_columns", "fseq_write_identity_columns",
         "fseq_write_founders_restored"]


@pytest.fixture(scope="module")
def build():
    return importlib.import_module("founder-sequences_amd.build")


@pytest.fixture(scope="module")
def pkg(build):
    build.build()
    return importlib.import_module("founder-sequences_amd")


def test_library_exports_the_entry_points(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pkg.EXPORTS and name not in pkg.DEBUG_EXPORTS
    assert lib.fseq_abi_version() == 5                       # (detected by symbol: no struct of the boundary changed)


def test_struct_layout_matches_header(pkg, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "fseq.h"\nint main(void){ printf("%zu\\n", sizeof(fseq_identity_summary)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size = int(subprocess.run([str(exe)], capture_output=True, check=True).stdout)
    assert size == C.sizeof(pkg.IdentitySummary) == 3 * 8 + 8


def test_null_and_ill_formed_arguments_fail_without_touching_a_device(pkg):
    lib = pkg.load_library()
    sm = pkg.IdentitySummary()
    h = C.c_void_p(0x1234)
    mask = (C.c_uint8 * 8)()
    perm = (C.c_uint32 * 4)()
    assert lib.fseq_identity_columns(None, mask, C.byref(sm)) == pkg.FSEQ_E_ARG
    p = pkg.Params(0, 0, 5, 0, 0, 0, 0)
    assert lib.fseq_create_without_identity_columns(None, C.byref(p), C.byref(h), C.byref(sm)) == pkg.FSEQ_E_ARG
    assert h.value is None                                   # (nothing is handed out)
    assert lib.fseq_create_without_identity_columns(None, None, C.byref(h), None) == pkg.FSEQ_E_ARG
    assert lib.fseq_create_without_identity_columns(None, C.byref(p), None, None) == pkg.FSEQ_E_ARG
    p = pkg.Params(0, 10, 5, 0, 0, 0, 0)                     # n is not the caller's to choose
    h = C.c_void_p(0x1234)
    assert lib.fseq_create_without_identity_columns(None, C.byref(p), C.byref(h), None) == pkg.FSEQ_E_ARG
    assert h.value is None
    assert lib.fseq_get_identity_columns(None, mask, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_write_identity_columns(None, None) == pkg.FSEQ_E_ARG
    assert lib.fseq_write_founders_restored(None, perm, None) == pkg.FSEQ_E_ARG


def test_front_end_names_the_options_and_refuses_what_is_out_of_scope(build, tmp_path):
    cli = build.build_cli()
    r = subprocess.run([cli, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--remove-identity-columns" in r.stdout and b"--output-identity-columns" in r.stdout
    common = [cli, "--input", str(tmp_path / "missing.txt"), "--segment-length-bound", "5", "--output-founders", str(tmp_path / "f")]
    # refused before any input is read: the input does not exist, and the message is the option's
    r = subprocess.run(common + ["--remove-identity-columns", "--gpus", "2"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--remove-identity-columns is not supported together with --gpus" in r.stderr
    assert b"Loading the input" not in r.stderr
    r = subprocess.run(common + ["--output-identity-columns", str(tmp_path / "i"), "--output-matches", str(tmp_path / "m")], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--remove-identity-columns is not supported together with --output-matches" in r.stderr
    assert b"Loading the input" not in r.stderr
    assert not (tmp_path / "i").exists() and not (tmp_path / "m").exists()


def run_host_chain(build, tmp_path, msa):
    """remove_identity_columns on the rows as files: (its stdout, the reduced rows it wrote or None when it wrote nothing)."""
    tools = dict(zip(build.AUX_TOOLS, build.build_aux()))
    src, dst = tmp_path / "in", tmp_path / "reduced"
    src.mkdir()
    dst.mkdir()
    names = []
    for i, row in enumerate(msa):
        (src / ("s%d" % i)).write_bytes(row.tobytes())
        names.append(str(src / ("s%d" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    r = subprocess.run([tools["remove_identity_columns"], "--input", str(tmp_path / "list.txt")], capture_output=True, cwd=str(dst), timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [np.frombuffer((dst / ("s%d" % i)).read_bytes(), dtype=np.uint8) for i in range(len(msa))]
    return r.stdout, np.array(rows), tools


CASES = [("mixed", 5, 300, 4, 0.6), ("two chunks", 3, 32768 + 40, 16, 0.6), ("three chunks", 12, 70000, 4, 0.6), ("exact chunk", 3, 32768, 2, 0.6),
         ("none", 4, 500, 4, 0.0), ("all", 4, 500, 4, 1.0), ("one row", 1, 77, 4, 0.5)]


@pytest.mark.parametrize("name,m,n,sigma,share", CASES, ids=[c[0] for c in CASES])
def test_model_is_the_host_tools(build, tmp_path, name, m, n, sigma, share):
    msa = im.random_case(len(name) + n, m, n, sigma, share)
    mask = im.identity_mask(msa)
    assert {"none": not mask.any(), "all": mask.all(), "one row": mask.all()}.get(name, mask.any() and not mask.all())
    out, reduced, tools = run_host_chain(build, tmp_path, msa)
    assert out == im.mask_text(mask)
    want = im.reduce_rows(msa, mask)
    assert reduced.shape == want.shape and np.array_equal(reduced, want)
    if mask.all():
        return
    # some founders over the reduced columns (here: a few reduced rows, reversed) restored from row 0's file
    founders = want[::-1][:3]
    (tmp_path / "founders.txt").write_bytes(b"".join(f.tobytes() + b"\n" for f in founders))
    (tmp_path / "mask.txt").write_bytes(out)
    back = tmp_path / "restored"
    back.mkdir()
    r = subprocess.run([tools["insert_identity_columns"], "--input", str(tmp_path / "founders.txt"), "--reference", str(tmp_path / "in" / "s0"),
                        "--identity-columns", str(tmp_path / "mask.txt")], capture_output=True, cwd=str(back), timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([np.frombuffer((back / str(i + 1)).read_bytes(), dtype=np.uint8) for i in range(len(founders))])
    assert np.array_equal(got, im.restore(founders, mask, msa[0]))
    assert np.array_equal(im.restore(want, mask, msa[0]), msa)       # (the rows themselves come back)
