"""The front end's --scan-segment-lengths, --output-scan and --max-founders on the card: the table is the library's scan, the
chosen bound is the one the table implies, and the founders are those of a plain run at that bound."""
import importlib
import subprocess

import pytest

import proto_length_scan as P

pytestmark = pytest.mark.gpu

LENGTHS = [5, 10, 20, 56, 97, 200, 1500, 4000]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("founder-sequences_amd.build").build_cli()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_cli")
    msa = P.case_msa("lds_resident")
    names = []
    for r in range(msa.shape[0]):
        f = d / ("s%03d.txt" % r)
        f.write_bytes(msa[r].tobytes())
        names.append(str(f))
    lst = d / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    return d, msa, str(lst)


@pytest.fixture(scope="module")
def table(pkg, inputs):
    _, msa, _ = inputs
    ctx = pkg.SegmentationContext(msa.shape[0], msa.shape[1], 20)
    ctx.set_sequences(msa)
    entries, _ = ctx.scan_segment_lengths(LENGTHS)
    ctx.close()
    return {int(e["segment_length"]): int(e["max_segment_size"]) for e in entries}


def test_table_equals_the_librarys_scan(cli, inputs, table):
    d, _, lst = inputs
    spec = ",".join(str(L) for L in reversed(LENGTHS + [20, 5]))         # any order, repeats
    r = subprocess.run([cli, "--input=" + lst, "--scan-segment-lengths=" + spec, "--output-scan=" + str(d / "t.tsv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = "SEGMENT_LENGTH\tMAX_SEGMENT_SIZE\n" + "".join("%d\t%d\n" % (L, table[L]) for L in sorted(LENGTHS))
    assert (d / "t.tsv").read_text() == want
    assert r.stdout == ""                                                # the scan alone writes no founders
    # the table on standard output by default, then the ordinary run at the given bound
    r = subprocess.run([cli, "--input=" + lst, "--scan-segment-lengths=5:20:5", "-s", "20", "-j", "greedy", "--output-founders=" + str(d / "f20.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[0] == "SEGMENT_LENGTH\tMAX_SEGMENT_SIZE" and [ln.split("\t")[0] for ln in r.stdout.splitlines()[1:]] == ["5", "10", "15", "20"]
    assert len((d / "f20.txt").read_bytes().splitlines()) == table[20]


def test_max_founders_picks_the_bound_the_table_implies(cli, inputs, table):
    d, _, lst = inputs
    long_sizes = sorted({table[L] for L in LENGTHS})
    K = long_sizes[len(long_sizes) // 2]
    chosen = max(L for L in LENGTHS if table[L] <= K)
    spec = ",".join(str(L) for L in LENGTHS)
    r = subprocess.run([cli, "--input=" + lst, "--scan-segment-lengths=" + spec, "--output-scan=" + str(d / "t2.tsv"), "--max-founders=%d" % K,
                        "-j", "greedy", "--output-founders=" + str(d / "fk.txt"), "--output-segments=" + str(d / "sk.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "segment length bound chosen: %d\n" % chosen in r.stderr
    p = subprocess.run([cli, "--input=" + lst, "-s", str(chosen), "-j", "greedy", "--output-founders=" + str(d / "fp.txt"), "--output-segments=" + str(d / "sp.txt")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (d / "fk.txt").read_bytes() == (d / "fp.txt").read_bytes() and (d / "sk.txt").read_bytes() == (d / "sp.txt").read_bytes()
    assert len((d / "fk.txt").read_bytes().splitlines()) == table[chosen] <= K


def test_no_bound_qualifies(cli, inputs, table):
    d, _, lst = inputs
    smallest = min(table[L] for L in (20, 56))
    r = subprocess.run([cli, "--input=" + lst, "--scan-segment-lengths=20,56", "--output-scan=" + str(d / "t3.tsv"), "--max-founders=%d" % (smallest - 1),
                        "--output-founders=" + str(d / "none.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "smallest maximum segment size seen was %d" % smallest in r.stderr
    assert not (d / "none.txt").exists()
