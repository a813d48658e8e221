"""-m gpu: the stream fan-out with mixed runs (mi_ravif_encoder.mixed_runs, Encoder.with_mixed_runs, cavif_mi --mixed-sizes): a run holds pictures of
different sizes.  The flag is a matter of speed alone: every file, status and release must be what the fan-out gives without it."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

from tests.helpers import mixed_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')


@pytest.fixture(scope='module')
def m():
    import cavif_rs_amd
    return cavif_rs_amd


def _raw_sources(m, e, items):
    """mi_ravif_encode_sources over (kind, object, channels) triples without raising: (status of the call, per-image statuses, files or None, released indices)"""
    E = m.encoder
    L = m.load_library()
    released = []

    def fetch(_user, i, src):
        (kind, it, channels), s = items[i], src.contents
        s.kind, s.jpeg, s.png = kind, None, None
        field = E._SOURCE_HANDLE_FIELD[kind & 0xFF]
        if field:
            setattr(s, field, it._h)
            s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = None, it.width, it.height, it.width, channels
        else:
            s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = it.ctypes.data, it.shape[1], it.shape[0], it.shape[1], channels
        return 0
    n = len(items)
    out, status = (E._EncodedImage * n)(), (C.c_int * n)()
    ec = e._c()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, E._FETCH_SOURCE(fetch), E._RELEASE(lambda _u, i: released.append(i)), None, out, status, None, 0)
    return rc, list(status), [E._take(o).avif_file if s == 0 else None for o, s in zip(out, status)], sorted(released)


def test_twelve_sources_of_five_sizes_and_every_kind(m, oracle):
    """host arrays, JPEG and PNG handles, a deep PNG, a managed and an oriented source, sizes alternating: index by index the files of the fan-out without the
    flag; the host arrays' files are the oracle's"""
    items = mc.stream_items(m)
    assert len(items) == 12 and len(set(mc.item_sizes(items))) == 5
    e = m.Encoder().with_quality(70).with_speed(10)
    off = _raw_sources(m, e, items)
    on = _raw_sources(m, e.with_mixed_runs(), items)
    assert off[0] == 0 and off[1] == [0] * 12 and off[3] == list(range(12))
    assert on[0] == 0 and on[1] == [0] * 12 and on[3] == list(range(12))
    assert [a == b for a, b in zip(on[2], off[2])] == [True] * 12
    for (kind, it, _), got in zip(items, on[2]):
        if kind == m.encoder.SOURCE_HOST:
            assert got == oracle.ravif_encode(it, quality=70, speed=10)[0]
    # the managed source was converted and the oriented one turned: neither is the file of its plain kind
    plain = _raw_sources(m, e.with_mixed_runs(), [(m.encoder.SOURCE_PNG, items[10][1], 3), (m.encoder.SOURCE_JPEG, items[5][1], 3)])
    assert plain[1] == [0, 0] and plain[2][0] != on[2][10] and plain[2][1] != on[2][5]


def test_encode_many_passes_the_flag_through(m, oracle):
    e = m.Encoder().with_quality(70).with_speed(10)
    assert e.with_mixed_runs()._c().mixed_runs == 1 and e._c().mixed_runs == 0 and e.with_mixed_runs().with_mixed_runs(False)._c().mixed_runs == 0
    images = [mc.rgb(8, 8), mc.rgb(200, 136), mc.rgb(37, 23), mc.rgb(8, 8, 1), mc.rgb(129, 101)]
    got = [x.avif_file for x in m.encode_many(e.with_mixed_runs(), images)]
    assert got == [oracle.ravif_encode(im, quality=70, speed=10)[0] for im in images]
    assert got == [x.avif_file for x in m.encode_many(e, images)]


def test_a_refused_source_fails_alone_with_the_status_it_has_today(m):
    """a PNG with an alpha channel described with 3 channels: InvalidArgument for that source, every other file as without it"""
    from tests.helpers import png_cases as pc
    E = m.encoder
    rng = np.random.default_rng(8)
    with_alpha = m.parse_png(pc.make_png(pc.random_samples(rng, 20, 12, 8, 6), 8, 6))
    items = [(E.SOURCE_HOST, mc.rgb(8, 8), 3), (E.SOURCE_PNG, with_alpha, 3), (E.SOURCE_HOST, mc.rgb(37, 23), 3), (E.SOURCE_HOST, mc.rgb(20, 12), 3)]
    e = m.Encoder().with_speed(10)
    off = _raw_sources(m, e, items)
    on = _raw_sources(m, e.with_mixed_runs(), items)
    assert off[:2] == (mc.INVALID, [0, mc.INVALID, 0, 0])
    assert on == off and on[2][1] is None and all(on[2][i] for i in (0, 2, 3)) and on[3] == [0, 1, 2, 3]


def test_a_picture_too_large_for_the_mixed_object_goes_the_per_shape_way(m):
    """one source: the worker's mixed object is made for 1 x 1920 x 1080, which a picture of 2000 x 1200 does not fit -- asked of a batch of that reference
    shape -- and the picture still comes out, with the bytes of the per-shape path"""
    e = m.Encoder().with_quality(60).with_speed(10)
    probe = m.BatchEncoder(e, 1, 1920, 1080, 3)
    assert probe.fits([(1920, 1080)]) and not probe.fits([(2000, 1200)])
    probe.close()
    big = mc.rgb(2000, 1200)
    on = m.encode_many(e.with_mixed_runs(), [big])[0].avif_file
    assert len(on) > 1000 and on == m.encode_many(e, [big])[0].avif_file


def test_cavif_mi_mixed_sizes_writes_the_same_files(m, tmp_path):
    from tests.helpers import png_cases as pc
    rng = np.random.default_rng(21)
    outs = {}
    for flag in ('', '--mixed-sizes'):
        d = tmp_path / ('on' if flag else 'off')
        d.mkdir()
        files = []
        rng = np.random.default_rng(21)
        for i, (w, h, ctype) in enumerate(((33, 50, 2), (8, 8, 2), (200, 136, 6), (37, 23, 2), (129, 101, 0), (72, 136, 2))):
            p = d / ('p%d.png' % i)
            p.write_bytes(pc.make_png(pc.random_samples(rng, w, h, 8, ctype), 8, ctype, seed=i))
            files.append(p)
        r = subprocess.run([CLI, '-q', '-s', '10'] + ([flag] if flag else []) + [str(f) for f in files], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[flag] = [f.with_suffix('.avif').read_bytes() for f in files]
    assert outs['--mixed-sizes'] == outs[''] and all(len(x) > 100 for x in outs['']) and len(set(outs[''])) == 6
