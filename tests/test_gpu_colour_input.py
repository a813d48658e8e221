"""-m gpu: colour-managed input on the MI355X through the product library -- the case table of tests/helpers/colour_cases.py (the kernels on 8-bit and deep
slots, files converted by their own description, refusals), one end-to-end case at 67 x 50 and a conversion ordered after a torch tensor's upload.  Every
comparison is for equality against tests/helpers/colour_ref.py.  Nothing is wider than 517 pixels."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'colour_cases.py')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, *prefixes):
    from tests.helpers.colour_cases import expected_rows
    want = expected_rows()
    for prefix in prefixes:
        mine = [r for r in rows if r['case'].startswith(prefix)]
        bad = [r for r in mine if not r['ok']]
        assert not bad, bad
        assert len(mine) == want[prefix], (prefix, [r['case'] for r in mine])


def test_the_library_bakes_the_restated_tables(table):
    _of(table, 'icc parses', 'png tables')


def test_slots_are_converted_in_place(table):
    _of(table, 'kernels')


def test_files_are_converted_by_their_own_description(table):
    _of(table, 'files png', 'files jpeg', 'files unchanged')


def test_conversions_are_refused_with_invalid_argument(table):
    _of(table, 'refused')


def test_encode_managed_gives_the_file_of_the_restated_pixels(table):
    """Encoder.encode_managed over a Display P3 PNG, 8-bit and deep, a PNG with alpha and gAMA, a JPEG with a profile; files that say nothing, sRGB, or carry an
    unsupported or malformed profile give the unmanaged file"""
    _of(table, 'e2e')


def test_managed_source_kinds_beside_the_others(table):
    """encode_many(managed=True) over a mixed list (a managed PNG, a managed JPEG, files with an unsupported and a malformed profile, a host array), the same list
    without the keyword, kinds 0 to 7 in one run of mi_ravif_encode_sources"""
    _of(table, 'sources')


def test_a_conversion_is_ordered_after_a_tensor_upload():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch')


def test_cli_color_managed_flag(tmp_path):
    """a directory of a Display P3 PNG, a P3 JPEG, a PNG with an unsupported profile, a 16-bit P3 PNG, a plain PNG and a PNG with a degenerate cHRM, 33 x 50.  Without --color-managed every
    file is today's (Encoder.encode_rgba(load_rgba(bytes))).  With it the files are those of the restated sRGB pixels; the unsupported profile and a gAMA file whose
    cHRM has a zero white point give today's files and one warning line each that names them; with --deep-png as well the 16-bit file is converted in its deep slot; -q silences the warning."""
    import numpy as np
    import cavif_rs_amd as m
    from tests.helpers import colour_cases as K
    cli = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
    S = K.mixed_sources()
    ref, opaque = S['ref'], S['opaque']
    src = tmp_path / 'in'
    src.mkdir()
    names = ('p3_png', 'p3_jpeg', 'cmyk_png', 'deep_png', 'plain_png', 'bad_chrm_png')
    files = []
    for name in names:
        p = src / (name + ('.jpg' if name.endswith('jpeg') else '.png'))
        p.write_bytes(S[name])
        files.append(p)
    aq = min((80.0 + 100.0) / 2.0, 80.0 + 80.0 / 4.0 + 2.0)                      # src/main.rs:115
    e = m.Encoder().with_quality(80.0).with_alpha_quality(aq).with_speed(4).with_alpha_color_mode('clean')
    old = [e.encode_rgba(m.load_rgba(f.read_bytes())).avif_file for f in files]
    jpeg_rgba = m.decode_jpeg(S['jp'])
    new = [e.encode_rgba(ref.convert8(opaque(S['s8']))).avif_file, e.encode_rgba(ref.convert8(jpeg_rgba)).avif_file, old[2],
           e.encode_rgba(ref.convert8(opaque((S['s16'] >> 8).astype(np.uint8)))).avif_file, old[4], old[5]]
    deep = list(new)
    b = m.BatchEncoder(e, 1, 33, 50, 4)                                        # the library's own deep file: an opaque 16-bit picture in a 4-channel batch
    b.upload(0, ref.convert16(S['s16']))
    b.encode()
    deep[3] = b.get(0).avif_file
    b.close()
    assert new[0] != old[0] and new[1] != old[1] and deep[3] != new[3]
    for k, (flags, want, warns) in enumerate(((['--color-managed'], new, 2), ([], old, 0), (['--color-managed', '--deep-png'], deep, 2), (['--color-managed', '-q', '--jpeg-ycbcr'], new, 0))):
        out = tmp_path / ('out%d' % k)
        r = subprocess.run([cli, '-o', str(out)] + flags + [str(f) for f in files], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for f, w_ in zip(files, want):
            assert (out / (f.stem + '.avif')).read_bytes() == w_, (flags, f.name)
        lines = [l for l in r.stderr.decode().splitlines() if l.startswith('warning:')]
        assert len(lines) == warns and sorted(('cmyk_png' in l and 'unsupported' in l, 'bad_chrm_png' in l and 'malformed' in l) for l in lines) == [(False, True), (True, False)][:warns], r.stderr
    assert b'--color-managed' in subprocess.run([cli], capture_output=True, timeout=60).stderr          # the usage text names the flag
