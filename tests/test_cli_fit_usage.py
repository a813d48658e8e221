"""cavif_mi --fit / --resize-filter: bad values leave through usage() before any file is read or any device is touched."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=60)


@pytest.mark.parametrize('bad', (['--fit', '0'], ['--fit', 'x'], ['--fit', '10x'], ['--fit', 'x10'], ['--fit', '0x0'], ['--fit', '-3'], ['--fit', '10x10x10'], ['--fit', '65537'], ['--fit', '1e3'], ['--fit'],
                                 ['--resize-filter', 'nearest'], ['--resize-filter', ''], ['--resize-filter']), ids=' '.join)
def test_bad_values_exit_through_usage(bad):
    assert os.path.exists(CLI), 'the command line is not built'
    r = _run(bad + ['missing.png'])
    assert r.returncode == 1 and b'error:' in r.stderr and b'usage: cavif_mi' in r.stderr and b'--fit WxH' in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize('good', (['--fit', '24'], ['--fit', '24x0'], ['--fit', '0x24'], ['--fit=2048x2048'], ['--fit', '65536'], ['--resize-filter', 'box'], ['--resize-filter', 'bilinear'],
                                  ['--resize-filter', 'bicubic'], ['--resize-filter=lanczos', '--fit', '7x9']), ids=' '.join)
def test_good_values_get_as_far_as_the_missing_file(good, tmp_path):
    assert os.path.exists(CLI), 'the command line is not built'
    r = _run(good + [str(tmp_path / 'missing.png')])
    assert r.returncode == 1 and b'usage:' not in r.stderr and b'Unable to read input image' in r.stderr, r.stderr[-500:]
