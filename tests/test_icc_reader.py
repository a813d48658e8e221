"""The colour descriptions of files on the CPU: icc_reader.h through mi_colour_transform_from_icc / _from_png, the PNG colour chunks and the JPEG APP2 segments
through the handles, inside the SIMT-emulated build of the product sources (host code only: nothing here launches a kernel).  The profiles, files and the
corruption sweep are tests/helpers/colour_cases.py; the expected tables are the restatement tests/helpers/colour_ref.py.  The same sweep runs once more over
icc_reader.h and the chunk and segment code in a stand-alone program built with -fsanitize=address,undefined (tests/kernels/colour_sweep_main.cpp)."""
import json
import os
import shutil
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rows():
    from tests import emu
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'colour_cases.py'), ROOT, 'icc'], env=emu.env(), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]


def check(rows, *prefixes):
    from tests.helpers.colour_cases import expected_rows
    want = expected_rows()
    for prefix in prefixes:
        mine = [r for r in rows if r['case'].startswith(prefix)]
        assert not [r for r in mine if not r['ok']], [r for r in mine if not r['ok']]
        assert len(mine) == want[prefix], (prefix, [r['case'] for r in mine])


def test_every_profile_parses_and_bakes_the_restated_tables(rows):
    """the profiles under test (curv with 0, 1 and n entries, para 0, 1, 3 and 4, a v4 header, a curve per channel): the matrix is the restatement's double
    matrix to the fixed-point step, and matrix, lin8, U, lin16 and out16 equal the restatement's integers"""
    check(rows, 'icc parses')


def test_profiles_of_other_kinds_are_unsupported(rows):
    check(rows, 'icc unsupported', 'python')


def test_the_corruption_sweep_gives_three_statuses_and_no_crash(rows):
    """truncation at every length below 132 + 12 tags, every tag offset and size at the 8 values around the profile's end, table counts 0xFFFFFFFF and
    len / 2 + 1, size fields off by one, a wrong signature, a missing tag, null pointers"""
    check(rows, 'icc sweep', 'icc refused', 'icc probes')


def test_gama_and_chrm_bake_the_restated_tables(rows):
    check(rows, 'png identity', 'png tables', 'png refused')


def test_png_chunks_and_jpeg_segments_are_kept_by_priority(rows):
    """iCCP over sRGB over gAMA (+ cHRM); broken chunks count as absent and never change the picture; the 4 MiB cap; APP2 segments in any order, and no
    profile when a number is missing or repeated or the counts disagree"""
    check(rows, 'png colour', 'jpeg profile', 'png cHRM')


def test_the_sweep_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """one stand-alone host program with its own main over icc_reader.h, png_reader.h's colour chunks and jpeg_reader.h's APP2 code: the corrupted profiles
    (raw, inside iCCP chunks and inside APP2 segments) written by colour_cases.py, each read from a heap copy of its exact length and carried through the
    description, cache key and bake helpers the stream workers use"""
    from tests.helpers import colour_cases as K
    from tests.helpers import png_cases as P
    import numpy as np
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed for the sanitizer build'
    exe = str(tmp_path / 'colour_sweep')
    src = os.path.join(ROOT, 'tests', 'kernels', 'colour_sweep_main.cpp')
    subprocess.check_call([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'cavif_rs_amd', 'csrc'), src, '-o', exe, '-lz'])
    base = P.make_png(P.random_samples(np.random.default_rng(1), 9, 5, 8, 2), 8, 2, seed=1)
    jp = K.jpeg_fixture('c420_4x4_q95_noise')
    blobs = []
    for name in ('p3 gamma 2.2', 'a curve per channel'):
        p = K.profile(name)
        cs = K.corruptions(p) + [p] + list(K.unsupported_profiles().values())
        blobs += [(0, c) for c in cs]
        blobs += [(1, K.with_chunks(base, K.iccp(c))) for c in cs[::7]] + [(2, K.with_app2(jp, K.app2(c, 1, 1))) for c in cs[::7]]
    half = len(p) // 2
    # bytes that are no profile and start with 'g', one byte and 74 bytes: raw, inside iCCP and inside APP2 (the stream workers' cache key must keep them a profile)
    for g in K.G_PROFILES:
        blobs += [(0, g), (1, K.with_chunks(base, K.iccp(g))), (2, K.with_app2(jp, K.app2(g, 1, 1))), (1, K.with_chunks(base, K.gama(100000), K.chrm(K.P3_CHRM)))]
    blobs += [(1, K.with_chunks(base, K.png_chunk(b'iCCP', body))) for body in (b'', b'n', b'n\0', b'n\0\0', b'n\0\0x', b'n' * 80 + b'\0\0', K.zlib.compress(p)[:-5])]
    blobs += [(1, K.with_chunks(base, K.png_chunk(b'gAMA', b'\0' * n), K.png_chunk(b'cHRM', b'\0' * (31 + n)), K.png_chunk(b'sRGB', b'\0' * n))) for n in (0, 1, 4, 5)]
    blobs += [(2, K.with_app2(jp, seg)) for seg in (b'\xff\xe2\x00\x02', b'\xff\xe2\x00\x0eICC_PROFILE\0', b'\xff\xe2\x00\x10ICC_PROFILE\0\x01\x01', K.app2(p[:half], 2, 2) + K.app2(p[half:], 1, 2))]
    path = str(tmp_path / 'blobs.bin')
    with open(path, 'wb') as fh:
        for kind, b in blobs:
            fh.write(bytes([kind]) + len(b).to_bytes(4, 'little') + b)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split()[:2] == ['blobs', str(len(blobs))], r.stdout
