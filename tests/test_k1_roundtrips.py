"""The tile search's block heads (one batch of loads per wave role: head_stage_issue / head_stage_consume), the contexts they keep for the transform-size trial, the
partition walker and its area copies (area_copy_dev: loads before stores, nothing saved or put back when the candidate evaluated last wins), through the SIMT
emulator: the product path must equal the oracle byte for byte on the cases of tests/helpers/k1_roundtrip_cases.py.
A stand-alone program (tests/kernels/k1_head_addr_main.cpp, built with the address and undefined-behaviour sanitizers) checks the address step of the split helpers
against restatements of the helpers they replaced: for every (availability, position, size) of a tile of 3 x 3 superblocks, each address equals the one the
earlier helper loaded from, or is the block's own cell / sample where the earlier helper loaded nothing."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from tests.helpers import k1_roundtrip_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_rows(oracle):
    from tests import emu
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'emu_walker_cases.py'), ROOT], env=emu.env(), capture_output=True, text=True, timeout=900)
    return p, [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]


def test_case_set_reaches_every_block_shape_and_every_8x8_winner(emu_rows):
    p, rows = emu_rows
    assert rows and rows[0] == {'case': 'inputs', 'ok': True}, p.stdout[-2000:] + p.stderr[-2000:]


def test_emulated_product_path_equals_oracle(emu_rows):
    p, rows = emu_rows
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert len(rows) == 1 + len(K.CASES) + 1 and all(r['ok'] for r in rows), rows      # the inputs line, the cases, the .avif file


def test_address_step_equals_the_earlier_helpers(tmp_path):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed for the stand-alone program'
    exe = str(tmp_path / 'k1_head_addr')
    subprocess.check_call([gxx, '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-w', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-I', os.path.join(ROOT, 'tests', 'emu', 'include'), '-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'kernels', 'k1_head_addr_main.cpp'), os.path.join(ROOT, 'tests', 'emu', 'emu_runtime.cpp'), '-o', exe, '-lz', '-lpthread', '-ldl'])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    assert 'mismatches 0' in p.stdout and 'out of bounds 0' in p.stdout, p.stdout[-3000:]
    checked = int(p.stdout.split('checked ')[1].split()[0])
    assert checked > 100000, p.stdout[-1000:]
