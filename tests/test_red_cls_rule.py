"""[r10] The direct-or-gather rule of the reduced column kernel's configurations on the CPU (red_cls_direct, csrc/fseq_redplan.hpp;
fseq_debug_red_cls_direct, include/fseq_debug.h): a configuration stages phase A's class columns itself where staged-column
buffers of the class width still fit the LDS and leave it as many resident workgroups per CU as the buffers sized for its rows.

The LDS figures are tabled by hand from the kernel's layout for every configuration of FSEQ_RED_CONFIGS at 2, 4 and 8 bits: two
staged-column buffers of whole kilobytes, each the bytes of the configuration's rows or -- class width -- the larger of those and a
class column of 12,288 keys (3,072 / 6,144 / 12,288 bytes).  The resident counts are the device's answer in a run; here they are
what 160 KB of LDS hold, or the workgroups the waves of a CU allow where that is fewer."""
import importlib
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("founder-sequences_amd")


# (threads, rows per thread, 16-bit, list wave) in the order of FSEQ_RED_CONFIGS (csrc/fseq_reduced.hip)
CONFIGS = [(64, 3, 0, 0), (64, 5, 0, 0), (64, 7, 0, 0), (256, 3, 0, 1), (256, 3, 0, 0), (256, 5, 0, 1), (256, 5, 0, 0), (512, 5, 0, 1), (512, 5, 0, 0),
           (512, 7, 0, 1), (512, 7, 0, 0), (1024, 5, 0, 1), (1024, 5, 0, 0), (512, 15, 1, 1), (1024, 7, 1, 1), (1024, 7, 1, 0),
           (1024, 8, 1, 1), (1024, 9, 1, 1), (1024, 9, 1, 0), (1024, 10, 1, 1), (1024, 10, 1, 0), (1024, 11, 1, 1), (1024, 11, 1, 0), (1024, 12, 1, 1)]
LDS = 160 * 1024
KEYS = 12288


def kb(x):
    return (x + 1023) // 1024 * 1024


def rows_of(T, E, ew):
    return (T - 64) * E if ew else T * E


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_lds_with_class_sized_buffers_for_every_configuration(pkg, bits):
    m, B = 100000, 100
    cls_ld = KEYS * bits // 8
    plan = pkg.red_plan_host(m, B, bits, False, [100])
    assert [(T, E, bool(ew)) for _, _, T, E, ew, _ in plan["configs"]] == [(T, E, bool(ew)) for T, E, _, ew in CONFIGS]
    for i, (T, E, pk, ew) in enumerate(CONFIGS):
        rows = rows_of(T, E, ew)
        assert plan["configs"][i][0] == rows
        per_rows = kb((rows * bits + 7) // 8)
        per_cls = kb(max((rows * bits + 7) // 8, cls_ld))
        lds_rows, lds_cls, _ = pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 1, 1)
        assert lds_cls - lds_rows == 2 * (per_cls - per_rows), (T, E, ew, lds_rows, lds_cls)
        # by hand: no configuration's rows reach a class column's bytes at any width (11,520 rows at most), so every one takes the
        # class column's; the largest need the same whole kilobytes for their rows (2 bits: from 8,193 rows on) and do not grow
        assert per_cls == cls_ld and (lds_cls > lds_rows) == (per_rows < cls_ld), (T, E, ew)
        if bits == 2:
            assert (lds_cls == lds_rows) == (rows > 8192), (T, E, ew)
        # ... and the rule, with the workgroups 160 KB of LDS hold at either size, bounded by the CU's 32 waves where that is fewer
        waves = max(1, 2048 // T) if T > 64 else 32
        r_rows, r_cls = min(LDS // lds_rows, waves), min(LDS // lds_cls, waves) if lds_cls <= LDS else 0
        want = lds_cls == lds_rows or (lds_cls <= LDS and r_cls >= 1 and r_cls >= r_rows)
        assert pkg.red_cls_direct_host(m, B, bits, cls_ld, i, r_rows, max(r_cls, 0))[2] == want, (T, E, ew, lds_rows, lds_cls, r_rows, r_cls)
        # one workgroup fewer: gather; the same count: direct -- whatever the sizes, as long as the class width fits
        if lds_cls == lds_rows:
            assert pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 1, 0)[2]        # (the same buffers: nothing to ask the device)
        elif lds_cls <= LDS:
            assert pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 3, 3)[2]
            assert not pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 3, 2)[2]
            assert not pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 1, 0)[2]
        else:
            assert not pkg.red_cls_direct_host(m, B, bits, cls_ld, i, 1, 1)[2]


def test_flagship_geometry_keeps_the_slim_configuration_direct(pkg):
    """Blocks of 814 columns, 2-bit symbols: 512 x 15 grows from 71,872 bytes by 2 KB (its rows need 2 KB a buffer, a class column
    3 KB) and two of it still fit a CU; 512 x 5 with a list wave (1 KB a buffer for its 2,240 rows) grows by 4 KB."""
    slim = CONFIGS.index((512, 15, 1, 1))
    lds_rows, lds_cls, direct = pkg.red_cls_direct_host(100000, 814, 2, 3072, slim, 2, 2)
    assert (lds_rows, lds_cls, direct) == (71872, 73920, True) and 2 * lds_cls <= LDS
    c = CONFIGS.index((512, 5, 0, 1))
    lds_rows, lds_cls, _ = pkg.red_cls_direct_host(100000, 814, 2, 3072, c, 1, 1)
    assert lds_cls - lds_rows == 4096


def test_arguments_are_checked(pkg):
    for args in [(0, 100, 2, 3072, 0, 1, 1), (100, 0, 2, 3072, 0, 1, 1), (100, 100, 3, 3072, 0, 1, 1), (100, 100, 2, 0, 0, 1, 1), (100, 100, 2, 3072, len(CONFIGS), 1, 1)]:
        with pytest.raises(pkg.FseqError) as e:
            pkg.red_cls_direct_host(*args)
        assert e.value.code == pkg.FSEQ_E_ARG


def test_rule_and_plan_under_sanitizers(tmp_path):
    """The header is host-only: tests/red_cls_rule_sanitized.cpp includes it alone and runs the rule and the per-block sources of
    plan_reduced under AddressSanitizer and UBSan."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "red_cls_rule_sanitized")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(os.path.dirname(here), "founder-sequences_amd", "csrc"), os.path.join(here, "red_cls_rule_sanitized.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "ok" in p.stdout
