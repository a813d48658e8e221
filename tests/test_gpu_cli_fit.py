"""-m gpu: cavif_mi --fit / --resize-filter on the MI355X: the files the command line writes over spliced JPEG and PNG files equal the library's files for the same
sources (encode_many with the same flags), and a file that fits the box equals the file written without --fit (tests/helpers/resize_orient_cases.py: run_cli)."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'resize_orient_cases.py')


def test_fit_writes_the_librarys_files_and_leaves_files_that_fit_alone():
    from tests.helpers.resize_orient_cases import CLI_CASES
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, 'cli'], env=env, capture_output=True, text=True, timeout=240)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith('cli')]) == CLI_CASES, [r['case'] for r in rows]
