"""The short constant division of the band means (const_div.hpp) is only as good as its proof: the table of proven
divisors in the source must be exactly what tools/verify_const_div.c printed (profiles/const_div_bands.txt), and the tool
itself must still build, find the dividends that are exact and find the ones that are not."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "const_div_bands.txt")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_band_div_table", os.path.join(ROOT, "tools", "gen_band_div_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def verifier(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    exe = tmp_path_factory.mktemp("const_div") / "verify_const_div"
    run = subprocess.run([cc, "-O2", "-mfma", "-fopenmp", "-ffp-contract=off", os.path.join(ROOT, "tools", "verify_const_div.c"),
                          "-o", str(exe), "-lm"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return str(exe)


def test_verifier_on_a_reduced_range(verifier):
    # d = 3 over two binades around 1.0: every quotient is the correctly rounded one
    out = subprocess.run([verifier, "--lo", "3f000000", "--hi", "40000000", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("d = 3 ")]
    assert len(line) == 1 and "exact on [3f000000, 40000000]" in line[0] and ", 0 mismatches" in line[0], out.stdout
    # d = 6 over the denormals: the tool must SEE the failures there (the quotient is a denormal), and +0 is exact
    out = subprocess.run([verifier, "--lo", "0", "--hi", "00ffffff", "6"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("d = 6 ")]
    assert len(line) == 1 and "+0 exact" in line[0], out.stdout
    assert int(re.search(r", (\d+) mismatches", line[0]).group(1)) > 0, line[0]
    # +inf fails for every divisor: inf - inf in the residual
    out = subprocess.run([verifier, "--lo", "7f7ffff0", "--hi", "7f800000", "3"], capture_output=True, text=True, timeout=600)
    assert "exact on [7f7ffff0, 7f7fffff]" in out.stdout and "above in [7f800000, 7f800000]" in out.stdout, out.stdout


def test_table_in_the_source_is_the_tools_output():
    gen = _gen()
    lo, hi = gen.guard_range()
    assert (lo, hi) == (0x0D800000, 0x7F7FFFFF)
    proven, seen = gen.proven_divisors(REPORT, lo, hi)
    assert open(gen.TABLE).read() == gen.render(proven), "band_div_proven.inc is not what tools/gen_band_div_table.py generates"
    in_source = [int(x) for x in re.findall(r"\b\d+\b", "".join(l for l in open(gen.TABLE) if not l.startswith("//")))]
    assert in_source == proven
    # the report covers the full dividend range for every divisor it lists, +0, denormals and +inf included
    assert "[00000000, 7f800000]" in open(REPORT).readline()
    # zero is in the report and is not proven; the headline plan's divisors all are
    assert 0.0 in seen and 0 not in proven
    headline = json.load(open(os.path.join(ROOT, "tests", "golden", "band_tables.json")))["B"]["divisors"]
    assert set(headline) <= set(proven), sorted(set(headline) - set(proven))
