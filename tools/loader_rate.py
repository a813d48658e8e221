"""PNG loader throughput per host core: mi_png_decode_rgba (inflate + unfilter + expansion to RGBA, what a loader thread did before PNG scanlines went to the
device) beside mi_png_parse (inflate alone, what it does now), on 1080p files of three forms: written like bench.py --end-to-end writes them (filter 0 on
every row, zlib level 1), and Pillow's default RGB and RGBA files (adaptive filters, Paeth on almost every row of a photograph).  The host budget of the
file fan-out (one MI355X takes ~260 files/s).  Usage: python tools/loader_rate.py [seconds per measurement, default 4]"""
import sys, time, ctypes as C, io, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cavif_rs_amd as m
from cavif_rs_amd.synth import synth_image
from scripts.gen_synth_png import write_png
L = m.load_library()
L.mi_png_decode_rgba.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
L.mi_png_parse.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
L.mi_free.argtypes = [C.c_void_p]
seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
d = tempfile.mkdtemp()
forms = {'synthetic (filter 0, zlib 1)': [], 'Pillow RGB': [], 'Pillow RGBA': []}
for i in range(4):
    img = synth_image(1920, 1080, index=i)
    p = os.path.join(d, 'a%d.png' % i); write_png(p, img); forms['synthetic (filter 0, zlib 1)'].append(open(p, 'rb').read())
    try:
        from PIL import Image
        b = io.BytesIO(); Image.fromarray(img, 'RGB').save(b, 'PNG'); forms['Pillow RGB'].append(b.getvalue())
        b = io.BytesIO(); Image.fromarray(synth_image(1920, 1080, index=i, alpha=True), 'RGBA').save(b, 'PNG'); forms['Pillow RGBA'].append(b.getvalue())
    except ImportError:
        pass


def decode(x):
    out = C.POINTER(C.c_uint8)(); w = C.c_uint32(); h = C.c_uint32()
    st = L.mi_png_decode_rgba(x, len(x), C.byref(out), C.byref(w), C.byref(h)); assert st == 0
    L.mi_free(out)


def parse(x):
    hnd = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32()
    st = L.mi_png_parse(x, len(x), C.byref(hnd), C.byref(w), C.byref(h), None); assert st == 0
    L.mi_png_scanlines_free(hnd)


for name, datas in forms.items():
    if not datas:
        continue
    print('%s: png bytes %s' % (name, [len(x) for x in datas]))
    rate = {}
    for what, fn in (('mi_png_decode_rgba', decode), ('mi_png_parse', parse)):
        n = 0; t = time.time()
        while time.time() - t < seconds:
            for x in datas:
                fn(x); n += 1
        dt = time.time() - t
        rate[what] = n / dt
        print('  %-18s %d calls in %.2f s: %.1f files/s per core, %.1f ms per 1080p file, %.1f MPix/s per core' % (what, n, dt, n / dt, 1e3 * dt / n, n * 1920 * 1080 / 1e6 / dt))
    print('  the loader sheds %.0f %% of its time per file' % (100 * (1 - rate['mi_png_decode_rgba'] / rate['mi_png_parse'])))
