"""Mixed-size batches (mi_batch_set_sizes): the cases tests/test_mixed_batch.py runs on the MI355X and tests/emu/mixed_cases.py runs on the
emulated library (TEST INFRASTRUCTURE).  Pictures are coded independently, so every file of a mixed run must equal, byte for byte, the oracle's file of that
picture alone; each case returns the list of what differed (empty: the case holds).  `m` is cavif_rs_amd, `oracle` tests/helpers/oracle."""
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.images import planes, rgba_gradient, rgba_noisy, rgba_opaque

UNSUPPORTED, INVALID = 2, 4

# a single superblock; less than one block; several superblocks in both directions with edges that are no multiples of 8; one block and a half; landscape; portrait
COLOUR_SIZES = [(64, 64), (8, 8), (129, 101), (17, 9), (200, 72), (72, 136)]
COLOUR_REFERENCE = (6, 256, 192)                      # cap, W, H: 6 x 12 superblocks reserved, the six pictures pad to 23
# (speed, bit depth, tiles_override, rdo_passes): the <= 16x16 class, the bottom-up 64x64 class, speed 10; frames of one launch that differ in tile count (the
# 8 x 8 picture keeps one tile); two-pass pricing; bit depth 8
COLOUR_SETTINGS = [(4, 10, 0, 1), (1, 10, 0, 1), (10, 10, 0, 1), (4, 10, 4, 1), (4, 10, 0, 2), (4, 8, 0, 1)]
ALPHA_REFERENCE = (4, 96, 80)                         # the cleaner's one-image scratch holds 96 x 80 pixels: 90 x 70 is the largest picture


def rgb(w, h, seed=None):
    return np.stack(planes(h, w, seed=w + h if seed is None else seed), -1).astype(np.uint8)


def colour_pictures():
    return [rgb(w, h) for w, h in COLOUR_SIZES]


def alpha_pictures():
    """64 x 64 with an alpha gradient, 40 x 24 opaque, 8 x 8 with alpha, 90 x 70 with noisy alpha (the cleaner does work)"""
    return [rgba_gradient(64, 64), rgba_opaque(40, 24), rgba_gradient(8, 8), rgba_noisy(90, 70)]


def sizes_of(images):
    return [(im.shape[1], im.shape[0]) for im in images]


def encoder(m, speed=4, depth=10, tiles=0, passes=1, quality=80.0, alpha_mode='clean'):
    e = m.Encoder().with_quality(quality).with_speed(speed).with_bit_depth(depth).with_rdo_passes(passes).with_alpha_color_mode(alpha_mode)
    return e._copy(tiles_override=tiles)


def mixed_batch(m, e, reference, images, channels):
    """a batch made for `reference` = (cap, W, H), laid out for `images` and holding them"""
    cap, w, h = reference
    b = m.BatchEncoder(e, cap, w, h, channels)
    assert b.fits(sizes_of(images)), 'the layout must fit its reference'
    b.set_sizes(sizes_of(images))
    for i, im in enumerate(images):
        b.upload(i, im)
    return b


def colour_case(m, oracle, speed, depth=10, tiles=0, passes=1):
    images = colour_pictures()
    b = mixed_batch(m, encoder(m, speed, depth, tiles, passes), COLOUR_REFERENCE, images, 3)
    b.encode()
    bad = []
    for i, im in enumerate(images):
        ref = oracle.ravif_encode(im, quality=80, speed=speed, depth=depth, tiles=tiles, rdo_passes=passes)[0]
        if b.get(i).avif_file != ref:
            bad.append('speed %d depth %d tiles %d passes %d: picture %d (%dx%d) differs from the oracle' % (speed, depth, tiles, passes, i, im.shape[1], im.shape[0]))
    if tiles:                                             # the frames of the launch do differ in tile count
        counts = b.num_tiles()
        if not counts > len(images):
            bad.append('tiles_override %d: %d tile jobs for %d pictures' % (tiles, counts, len(images)))
    b.close()
    return bad


def alpha_case(m, oracle, mode):
    """mode 0 dirty, 1 clean, 2 premultiplied"""
    images = alpha_pictures()
    name = ('dirty', 'clean', 'premultiplied')[mode]
    b = mixed_batch(m, encoder(m, 6, 10, quality=66.0, alpha_mode=name).with_alpha_quality(88.0), ALPHA_REFERENCE, images, 4)
    b.encode()
    bad = []
    for i, im in enumerate(images):
        ref, color, alpha = oracle.ravif_encode(im, quality=66, alpha_quality=88, speed=6, depth=10, alpha_mode=mode)
        got = b.get(i)
        if got.avif_file != ref or (got.color_byte_size, got.alpha_byte_size) != (color, alpha):
            bad.append('alpha mode %s: picture %d differs from the oracle' % (name, i))
        if b.uses_alpha(i) != (alpha > 0):                    # per picture: the oracle's file of this picture carries an alpha frame or does not
            bad.append('alpha mode %s: uses_alpha(%d) is %r' % (name, i, b.uses_alpha(i)))
    if mode != 2 and [b.uses_alpha(i) for i in range(4)] != [True, False, True, True]:      # (the unassociated modes drop the alpha of an opaque picture)
        bad.append('alpha mode %s: uses_alpha is not per picture' % name)
    b.close()
    return bad


def status_of(call):
    try:
        call()
        return 0
    except Exception as ex:                                # AvifError: its code
        return getattr(ex, 'code', repr(ex))


def fit_rule_case(m, oracle):
    """the fit rule, derived from what a batch reserves and not tuned to it"""
    bad = []
    e = encoder(m, 10)
    b = m.BatchEncoder(e, 4, 64, 64, 3)
    foot = b._L.mi_batch_footprint(b._h)
    # 2048 samples fit the slots, but the padded plane of 64 x 2048 is 32 superblocks against the four reserved
    if b.fits([(1, 2048)]) is not False or status_of(lambda: b.set_sizes([(1, 2048)])) != UNSUPPORTED:
        bad.append('4 x 64x64: 1 x 2048 must be Unsupported')
    if b.fits([(8, 8)] * 5) is not False or status_of(lambda: b.set_sizes([(8, 8)] * 5)) != UNSUPPORTED:
        bad.append('4 x 64x64: five pictures must be Unsupported')
    if status_of(lambda: b.fits([(0, 5)])) != INVALID or status_of(lambda: b.set_sizes([(0, 5)])) != INVALID or status_of(lambda: b.fits([])) != INVALID:
        bad.append('4 x 64x64: a zero extent and an empty layout must be InvalidArgument')
    if b.image_size(3) != (64, 64) or b.count != 4:
        bad.append('a refused layout changed the batch')
    b.set_sizes([(64, 64), (8, 8)])
    if b._L.mi_batch_footprint(b._h) != foot or b.image_size(1) != (8, 8) or status_of(lambda: b.image_size(2)) != INVALID:
        bad.append('4 x 64x64: footprint or image_size after set_sizes')
    b.close()
    # larger than the reference, but its padded plane of 256 x 128 is half the reserve
    b = m.BatchEncoder(e, 4, 128, 128, 3)
    foot = b._L.mi_batch_footprint(b._h)
    im = rgb(250, 120)
    if not b.fits([(250, 120)]):
        bad.append('4 x 128x128: 250 x 120 must fit')
    else:
        b.set_sizes([(250, 120)])
        b.upload(0, im)
        b.encode()
        if b.get(0).avif_file != oracle.ravif_encode(im, quality=80, speed=10, depth=10)[0]:
            bad.append('4 x 128x128: 250 x 120 differs from the oracle')
        if b._L.mi_batch_footprint(b._h) != foot:
            bad.append('4 x 128x128: the footprint changed')
    b.close()
    return bad


def stream_items(m):
    """(kind, object, channels of the slot) triples for encoder._encode_sources: twelve sources of five sizes between 8 x 8 and 200 x 136 in an order that
    alternates sizes -- host arrays, JPEG and PNG handles, one deep PNG, one managed source (a gAMA file) and one oriented source (a JPEG turned upside down, which
    keeps its size) -- reusing the JPEG fixtures and the file writers of the PNG, colour and orientation tests.  All go into 3-channel slots, so they share runs."""
    from cavif_rs_amd import encoder as E
    from tests.helpers import png_cases as pc
    from tests.helpers import colour_cases as cc
    from tests.helpers import orient_ref as R
    rng = np.random.default_rng(5)

    def jpeg(name):
        return m.parse_jpeg(cc.jpeg_fixture(name))

    def png_bytes(w, h, depth=8, **kw):
        return pc.make_png(pc.random_samples(rng, w, h, depth, 2), depth, 2, **kw)
    items = [(E.SOURCE_HOST, rgb(8, 8)), (E.SOURCE_JPEG, jpeg('c444_37x23_q30')), (E.SOURCE_HOST, rgb(200, 136)), (E.SOURCE_PNG, m.parse_png(png_bytes(33, 50))),
             (E.SOURCE_HOST, rgb(37, 23, 1)), (E.SOURCE_JPEG | E.SOURCE_ORIENTED, m.parse_jpeg(R.splice_jpeg(cc.jpeg_fixture('c420_33x50_q30_opt'), R.exif_blob(3, 'MM')))), (E.SOURCE_PNG, m.parse_png(png_bytes(8, 8, filters=4))),
             (E.SOURCE_HOST, rgb(160, 96)), (E.SOURCE_JPEG_YCBCR, jpeg('c420_160x96_qt16')), (E.SOURCE_PNG_DEEP, m.parse_png(png_bytes(37, 23, 16, interlace=1))),
             (E.SOURCE_PNG_MANAGED, m.parse_png(cc.with_chunks(png_bytes(200, 136, seed=3), cc.gama(55555)))), (E.SOURCE_HOST, rgb(33, 50, 2))]
    return [(kind, it, 3) for kind, it in items]


def item_sizes(items):
    from cavif_rs_amd import encoder as E
    return [(it.shape[1], it.shape[0]) if kind == E.SOURCE_HOST else (it.width, it.height) for kind, it, _ in items]


# ---------------------------------------------------------------- pictures in device memory
class HostView:
    """a picture behind __cuda_array_interface__ for a library whose device memory is host memory (the emulated one)"""

    def __init__(self, a):
        self._keep = a
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr='|u1', data=(a.ctypes.data, False), version=2, strides=a.strides)


def host_view(a, crop):
    return HostView(a[crop])


def torch_view(a, crop):
    import torch
    return torch.from_numpy(a).cuda()[crop]


DEVICE_SIZES = [(20, 12), (37, 23), (33, 50), (9, 5)]
FILL = 0xA5


def device_cases(m, view):
    """{'layout': [...], 'range': [...]}: what differed.  view(array, crop) -> an object with __cuda_array_interface__ that shows array[crop] in device memory"""
    out = {'layout': [], 'range': []}
    b = m.BatchEncoder(m.Encoder().with_speed(10), 4, 64, 64, 3)

    def fill(sizes):
        b.set_sizes(sizes)
        for k, (w, h) in enumerate(sizes):
            b.upload(k, np.full((h, w, 3), FILL + k, np.uint8))

    def kept(sizes, touched):
        return all((b.read_input(k) == FILL + k).all() and b.read_input(k).shape == (h, w, 3) for k, (w, h) in enumerate(sizes) if k not in touched)
    # a crop of a larger array: rows 7 pixels longer than the picture, a row above and below
    fill(DEVICE_SIZES)
    src = rgb(33, 50, 4)
    big = np.zeros((52, 40, 3), np.uint8)
    big[1:51, 7:, :] = src
    b.upload_device(2, view(big, (slice(1, 51), slice(7, 40))))
    if not np.array_equal(b.read_input(2), src):
        out['layout'].append('the slot does not hold the view')
    if not kept(DEVICE_SIZES, {2}):
        out['layout'].append('a neighbour changed')
    # the range rule
    two = np.ascontiguousarray(np.stack([rgb(37, 23, 1), rgb(37, 23, 2)]))
    fill(DEVICE_SIZES)
    if status_of(lambda: b.upload_device(1, view(two, slice(None)))) != INVALID:      # slot 1 is 37 x 23, slot 2 is 33 x 50
        out['range'].append('two neighbours of different size must be InvalidArgument')
    if not kept(DEVICE_SIZES, set()):
        out['range'].append('a refused call wrote')
    sizes = [(9, 5), (37, 23), (37, 23), (20, 12)]
    fill(sizes)
    if status_of(lambda: b.upload_device(1, view(two, slice(None)))) != 0:
        out['range'].append('two equal neighbours inside a mixed layout must be taken')
    elif not (np.array_equal(b.read_input(1), two[0]) and np.array_equal(b.read_input(2), two[1]) and kept(sizes, {1, 2})):
        out['range'].append('two equal neighbours: the slots')
    b.close()
    return out


if __name__ == '__main__':                                 # python tests/helpers/mixed_cases.py ROOT torch: device_cases over torch views, one JSON line
    import json
    import torch                                           # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
    torch.zeros(1).cuda()
    import cavif_rs_amd
    print(json.dumps(device_cases(cavif_rs_amd, torch_view)), flush=True)
