"""The list budget's surface on CPU (fseq_set_list_memory, fseq_debug_list_windows): exported, bound, argument checks, and
the command line's --list-memory option, refused before the input is opened when it cannot apply."""
import ctypes as C
import importlib
import subprocess

import pytest


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    build = importlib.import_module("founder-sequences_amd.build")
    return build.build_cli()


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, timeout=300)


def test_new_symbols_are_exported_and_bound(pkg):
    assert "fseq_set_list_memory" in pkg.EXPORTS and "fseq_set_list_memory" not in pkg.DEBUG_EXPORTS
    assert "fseq_debug_list_windows" in pkg.EXPORTS and "fseq_debug_list_windows" in pkg.DEBUG_EXPORTS
    lib = pkg.load_library()
    assert hasattr(lib, "fseq_set_list_memory") and hasattr(lib, "fseq_debug_list_windows")
    assert lib.fseq_abi_version() == 5
    for name in ("set_list_memory", "list_windows"):
        assert callable(getattr(pkg.SegmentationContext, name))


def test_null_context_is_an_argument_error(pkg):
    lib = pkg.load_library()
    assert lib.fseq_set_list_memory(None, 1 << 30) == 1                # FSEQ_E_ARG
    assert lib.fseq_set_list_memory(None, 0) == 1
    b, cols, w, mw = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert lib.fseq_debug_list_windows(None, C.byref(b), C.byref(cols), C.byref(w), C.byref(mw)) == 1


def test_help_lists_the_option(cli):
    r = run(cli, "--help")
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    i = next(k for k, ln in enumerate(lines) if "--gpus=N" in ln)
    assert any("--list-memory=MIB" in ln for ln in lines[i:i + 3])      # beside --gpus


@pytest.mark.parametrize("value", ["abc", "-1", "12x", "", "-0"])
def test_bad_values_exit_before_the_input_is_opened(cli, tmp_path, value):
    missing = str(tmp_path / "does-not-exist.txt")
    r = run(cli, "-i", missing, "-s", "5", "--list-memory=" + value)
    assert r.returncode == 1
    assert b"The list memory must be a non-negative number of MiB." in r.stderr
    assert b"Unable to open the input file" not in r.stderr and b"Loading the input" not in r.stderr


def test_list_memory_with_several_gpus_is_refused(cli, tmp_path):
    missing = str(tmp_path / "does-not-exist.txt")
    r = run(cli, "-i", missing, "-s", "5", "--list-memory=1024", "--gpus", "2")
    assert r.returncode == 1
    assert b"--list-memory is not supported together with --gpus > 1." in r.stderr
    assert b"Unable to open the input file" not in r.stderr and b"Loading the input" not in r.stderr


def test_good_values_get_as_far_as_the_input(cli, tmp_path):
    missing = str(tmp_path / "does-not-exist.txt")
    for value in ("0", "4096"):
        r = run(cli, "-i", missing, "-s", "5", "--list-memory=" + value)
        assert r.returncode == 1 and b"Unable to open the input file" in r.stderr, value
    r = run(cli, "-i", missing, "-s", "5", "--list-memory=4096", "--gpus", "1")
    assert b"--list-memory is not supported" not in r.stderr
