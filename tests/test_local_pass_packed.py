"""The packed local pass of phase C's partition step (csrc/fseq_localpass.hpp) on the host: the text the device runs, with its two
instructions restated in plain C++, against the plain pass -- four running maxima, a compare and two selects per row and symbol.

tests/local_pass_packed_main.cpp holds the cases, for 11, 12 and 15 rows a thread: every symbol pattern of five rows (symbols
0 .. 4) with every choice of values from {0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF}; 100,000 seeded random threads; one symbol only,
each symbol absent, alternating symbols, one to fourteen trailing unused positions, all values equal, strictly falling, strictly
rising.  Values with bit 15 set are what no alignment of the suite reaches (ids stay below 16,384 + B): a signed packed maximum
would pass every end-to-end test and fails here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (11, 12, 15)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("local_pass") / "local_pass_packed"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "founder-sequences_amd", "csrc"),
                    os.path.join(ROOT, "tests", "local_pass_packed_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def runs(program):
    """The three programs side by side: {E: (exit status, stdout, stderr)}."""
    procs = {E: subprocess.Popen([program, str(E)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for E in ROWS}
    out = {}
    for E, p in procs.items():
        so, se = p.communicate()
        out[E] = (p.returncode, so, se)
    return out


@pytest.mark.parametrize("E", ROWS)
def test_packed_pass_is_the_plain_pass(runs, E):
    rc, so, se = runs[E]
    assert rc == 0, se
    words = so.split()
    # five rows: (4 symbols x 6 values + unused) ^ 5 cases; 100,000 random threads; the named ones on top
    assert words[0] == "ok" and int(words[1]) > 25 ** 5 + 100000


def test_program_refuses_other_row_counts(program):
    assert subprocess.run([program, "13"], capture_output=True).returncode == 2
