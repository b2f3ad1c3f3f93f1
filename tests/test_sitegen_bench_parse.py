"""tools/sitegen_bench.py reads ntsmSiteGen's -V lines: the line of the substitution scan and the longer one that -g prints
(three window counts) must both parse, field for field.  The lines are the program's own format strings filled in."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TIME = "Time: genome 302.2 ms, step 1 19615.1 ms, step 2 8222.1 ms, candidate files 3047.4 ms, step 3 4467.1 ms; 999690 SNPs, 24036010 candidates\n"
HEAD = ("Device: table build 4771.2 ms, table upload 152.2 ms (2737.2 MB), stage 38.4 ms, upload 19.0 ms, scan kernel 568.4 ms in 16 launches "
        "(8 full: 69.0 .. 73.4 ms each); ")
PLAIN = HEAD + "1073639701 windows, 3220919103 bitmap tests, 8556491964 probes\n"
GAPS = HEAD + "1073639701 windows (1073634327 of k + 1 bases, 1073645075 of k - 1), 7515483281 bitmap tests, 20427257923 probes\n"


def bench():
    spec = importlib.util.spec_from_file_location("sitegen_bench", os.path.join(ROOT, "tools", "sitegen_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_both_verbose_lines_parse():
    parse_v = bench().parse_v
    plain, gaps = parse_v("Processed 1 SNPs.\n" + PLAIN + TIME), parse_v(GAPS + TIME)
    for got in (plain, gaps):
        assert (got["scan_kernel_ms"], got["launches"], got["full_launches"]) == (568.4, 16, 8)
        assert (got["full_launch_ms_min"], got["full_launch_ms_max"], got["table_mb"]) == (69.0, 73.4, 2737.2)
        assert (got["windows"], got["step1_ms"], got["candidates"]) == (1073639701, 19615.1, 24036010)
    assert "windows_long" not in plain and "windows_short" not in plain
    assert (plain["bitmap_tests"], plain["probes"]) == (3220919103, 8556491964)
    assert (gaps["windows_long"], gaps["windows_short"]) == (1073634327, 1073645075)
    assert (gaps["bitmap_tests"], gaps["probes"]) == (7515483281, 20427257923)
