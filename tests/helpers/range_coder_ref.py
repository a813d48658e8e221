"""A plain reference for the entropy kernel's coder (K4, cavif_rs_amd/csrc/tile_entropy.h) -- test infrastructure only.

* `encode`: the AV1 range encoder (libaom od_ec_encode_q15, od_ec_enc_done) over the kernel's record formats, with `low` kept as one unbounded Python
  integer: no pre-carry units, no carry step -- the bytes are read off the exact final number.
* CDF adaptation per spec 8.3.2 on the inverse-CDF storage of the kernel and the oracle.
* `decode`: the spec's symbol decoder (8.2.2 init_symbol, 8.2.6 read_symbol with its adaptation, read_bool), written on the spec's own (non-inverse) CDFs.
* `kernel_units`: the pre-carry units the kernel hands to its carry scan, modelled from the same symbols (only to check what the harness stores, and to
  prove which carry chains a stream reaches).
* Seeded stream generators.  The property a stream exists for is asserted on the reference output: by the generator (the byte runs, the carry chains)
  or by tests/test_k4_coder.py::test_streams_reach_the_coder_hard_cases (phases, fills, counters, rows).

Records (tile_entropy.h): bits 31..30 = 00 an adaptive symbol (bits 0..15 the CDF row's offset, 16..19 the symbol, 20..23 the alphabet size - 1); with bit 29
the partition-edge bool of that row (bit 16 = has_cols); 01 bounds (bits 0..9 fl >> 6, 10..19 fh >> 6, 20..23 N - 1 - s).  No numpy on the arithmetic path.
"""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---------------------------------------------------------------- records
def rec_sym(off, s, ns):
    assert 0 <= s < ns <= 16 and 0 <= off < 65536
    return off | (s << 16) | ((ns - 1) << 20)


def rec_pedge(off, has_cols):
    return off | ((1 if has_cols else 0) << 16) | 0x20000000


def rec_bounds(fl6, fh6, nms):
    return 0x40000000 | fl6 | (fh6 << 10) | (nms << 20)


def rec_bit(b):
    return rec_bounds(256, 0, 0) if b else rec_bounds(512, 256, 1)


# partitions 2, 3, 4, 6, 7, 9 (has_cols) or 1, 3, 4, 5, 6, 8: the ones that split the block the way the frame edge needs (oracle write_partition)
PEDGE_SETS = {1: (2, 3, 4, 6, 7, 9), 0: (1, 3, 4, 5, 6, 8)}


def pedge_psum(cdf, off, has_cols):
    """P(the partitions that split this way) from the inverse-CDF row as it stands, modulo 2^32 like the C arithmetic."""
    return sum(((cdf[off + q - 1] if q > 0 else 32768) - cdf[off + q]) for q in PEDGE_SETS[1 if has_cols else 0]) & 0xFFFFFFFF


def adapt(cdf, off, s, ns):
    """spec 8.3.2 on an inverse CDF: rate = 3 + (cnt > 15) + (cnt > 31) + min(floor(log2 N), 2); the counter saturates at 32."""
    cnt = cdf[off + ns]
    rate = 3 + (cnt > 15) + (cnt > 31) + min(ns.bit_length() - 1, 2)
    for i in range(ns - 1):
        if i < s:
            cdf[off + i] += (32768 - cdf[off + i]) >> rate
        else:
            cdf[off + i] -= cdf[off + i] >> rate
    cdf[off + ns] = min(cnt + 1, 32)


def bounds_of(rec, cdf):
    """(fl, fh, N - 1 - s) the record codes with, adapting the row of an adaptive symbol.  fl = 32768: the first symbol of its alphabet."""
    off = rec & 0xFFFF
    if rec >> 30 == 0 and rec & 0x20000000:
        psum = pedge_psum(cdf, off, (rec >> 16) & 1)
        return (psum & 0xFFFF), 0, 0                  # symbol 1 of the inverse CDF (psum, 0) -- the oracle stores psum as a 16-bit entry
    if rec >> 30 == 0:
        s, ns = (rec >> 16) & 15, ((rec >> 20) & 15) + 1
        assert s < ns
        fl, fh = (cdf[off + s - 1] if s > 0 else 32768), cdf[off + s]
        adapt(cdf, off, s, ns)
        return fl, fh, ns - 1 - s
    assert rec >> 30 == 1, 'record %08x' % rec
    return (rec & 1023) << 6, ((rec >> 10) & 1023) << 6, (rec >> 20) & 15


# ---------------------------------------------------------------- encoder
class Coded:
    """What the reference made of a stream: bytes, final table, and per symbol (delta, d) -- low += delta at the window, then the window moves d bits."""
    def __init__(self, data, cdf, steps, tbits):
        self.data, self.cdf, self.steps, self.tbits = data, cdf, steps, tbits


def encode(records, cdf0):
    cdf = list(cdf0)
    rng, low, tbits, steps = 0x8000, 0, 0, []
    for rec in records:
        fl, fh, nm = bounds_of(rec, cdf)
        r8 = rng >> 8
        v = ((r8 * (fh >> 6)) >> 1) + 4 * nm
        if fl < 32768:
            u = ((r8 * (fl >> 6)) >> 1) + 4 * (nm + 1)
            delta, nr = rng - u, u - v
        else:
            delta, nr = 0, rng - v
        assert 4 <= nr < 65536, 'record %08x leaves no range' % rec
        d = 16 - nr.bit_length()
        low = (low + delta) << d                       # one exact number: bit 0 of the window is bit 0 of `low`
        rng, tbits = nr << d, tbits + d
        steps.append((delta, d))
    # od_ec_enc_done: low rounded up to a multiple of 2^14 with bit 14 set; bit 14 of the window is stream bit T (bit 0 = the top bit of byte 0)
    e = ((low + 0x3FFF) & ~0x3FFF) | 0x4000
    nb = (tbits >> 3) + 1
    lsb = 7 + (tbits & 7)                              # the window bit that lands on the last byte's bit 0
    assert e & ((1 << lsb) - 1) == 0
    x = e >> lsb
    assert x >> (8 * nb) == 0, 'carry out of the stream'
    return Coded(x.to_bytes(nb, 'big'), cdf, steps, tbits)


def kernel_units(steps, tbits):
    """The kernel's pre-carry units (RangeEncDev, re_finish_dev) from the reference's (delta, d): unit k = the low byte of accumulator k + what
    accumulators k + 1, k + 2 hold above their low bytes; the accumulators get every delta's three byte slices at the bit the window stands at."""
    q = 14 + tbits
    kend = q >> 3
    acc = [0] * (kend + 3)
    t = 0
    for delta, d in steps:
        qq = 14 + t
        kk, val = qq >> 3, delta << (7 - (qq & 7))
        for j, part in ((0, val & 255), (1, (val >> 8) & 255), (2, val >> 16)):
            if part:
                assert kk - j >= 0
                acc[kk - j] += part
        t += d
    sh = 7 - (q & 7)
    V = sum(acc[kend - j] << (8 * j) for j in range(4) if kend >= j)
    A, B = 0x3FFF << sh, 0x4000 << sh
    add = (((V + A) & ~(B - 1)) | B) - V
    acc[kend] += add & 255
    acc[kend - 1] += (add >> 8) & 255
    if kend >= 2:
        acc[kend - 2] += add >> 16
    return [(acc[k] & 255) + ((acc[k + 1] >> 8) & 255) + (acc[k + 2] >> 16) for k in range(kend + 1)]


def resolve_units(units, nb):
    """Bytes from the units by the plain carry loop (the oracle's re_finish): a check on kernel_units."""
    out, carry = [0] * len(units), 0
    for i in range(len(units) - 1, -1, -1):
        carry += units[i]
        out[i] = carry & 255
        carry >>= 8
    assert carry == 0 and all(b == 0 for b in out[nb:])
    return bytes(out[:nb])


def carry_chains(units):
    """Runs of units the kernel's scan sees as `propagate` (byte + the high part of the unit after it == 255) that receive a carry from below: their lengths."""
    n = len(units)
    t = [(units[i] & 255) + (units[i + 1] >> 8 if i + 1 < n else 0) for i in range(n)]
    carry_in = [0] * (n + 1)                    # carry into unit i from the units after it
    c = 0
    for i in range(n - 1, -1, -1):
        carry_in[i] = c
        c = 1 if t[i] + c >= 256 else 0
    chains, i = [], 0
    while i < n:
        if t[i] == 255:
            j = i
            while j + 1 < n and t[j + 1] == 255:
                j += 1
            if carry_in[j]:
                chains.append((i, j - i + 1))
            i = j + 1
        else:
            i += 1
    return chains


# ---------------------------------------------------------------- decoder (spec 8.2, on the spec's own CDFs: cdf[i] = 32768 * P(symbol <= i))
class SpecDecoder:
    def __init__(self, data, cdf_inverse):
        self.data, self.pos = bytes(data), 0        # pos: bits read so far
        self.cdf = {}                               # row offset -> spec CDF (N entries + counter), made on first use from the inverse table
        self.inv0 = cdf_inverse
        sz = len(self.data)
        nbits = min(sz * 8, 15)
        buf = self._bits(nbits)
        self.val = ((1 << 15) - 1) ^ (buf << (15 - nbits))
        self.rng = 1 << 15
        self.maxbits = 8 * sz - 15
        self.consumed = 15                          # window bits used so far (past the data's end too)

    def _bits(self, n):
        v = 0
        for _ in range(n):
            byte = self.data[self.pos >> 3] if (self.pos >> 3) < len(self.data) else 0
            v = (v << 1) | ((byte >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def row(self, off, ns):
        if off not in self.cdf:
            self.cdf[off] = [32768 - self.inv0[off + i] for i in range(ns)] + [self.inv0[off + ns]]
        return self.cdf[off]

    def read_symbol(self, cdf, adapt_row=True):
        n = len(cdf) - 1
        cur, sym = self.rng, -1
        while True:
            sym += 1
            prev = cur
            f = (1 << 15) - cdf[sym]
            cur = ((self.rng >> 8) * (f >> 6) >> 1) + 4 * (n - sym - 1)
            if self.val >= cur:
                break
        self._renormalize(prev, cur)
        if adapt_row:
            self._adapt(cdf, n, sym)
        return sym

    def _renormalize(self, prev, cur):
        self.rng = prev - cur
        self.val -= cur
        bits = 15 - (self.rng.bit_length() - 1)
        self.rng <<= bits
        numbits = min(bits, max(0, self.maxbits))
        new = self._bits(numbits)
        self.val = (new << (bits - numbits)) ^ (((self.val + 1) << bits) - 1)
        self.maxbits -= bits
        self.consumed += bits

    @staticmethod
    def _adapt(cdf, n, sym):
        rate = 3 + (cdf[n] > 15) + (cdf[n] > 31) + min((n).bit_length() - 1, 2)
        tmp = 0
        for i in range(n - 1):
            tmp = (1 << 15) if i == sym else tmp
            if tmp < cdf[i]:
                cdf[i] -= (cdf[i] - tmp) >> rate
            else:
                cdf[i] += (tmp - cdf[i]) >> rate
        cdf[n] += cdf[n] < 32

    def read_bool(self):
        return self.read_symbol([1 << 14, 1 << 15, 0], adapt_row=False)

    def read_pedge(self, off, has_cols):
        c = self.row(off, 10)
        psum = sum(c[q] - (c[q - 1] if q > 0 else 0) for q in PEDGE_SETS[has_cols])
        return self.read_symbol([(1 << 15) - psum, 1 << 15, 0], adapt_row=False)

    def read_record(self, rec):
        """The value the record codes: a symbol, the bool of a partition edge, a bit of a K4_BIT record."""
        if rec >> 30 == 0 and rec & 0x20000000:
            return self.read_pedge(rec & 0xFFFF, (rec >> 16) & 1)
        if rec >> 30 == 0:
            return self.read_symbol(self.row(rec & 0xFFFF, ((rec >> 20) & 15) + 1))
        if rec in (rec_bit(0), rec_bit(1)):
            return self.read_bool()
        return self.read_bounds((rec & 1023) << 6, ((rec >> 10) & 1023) << 6, (rec >> 20) & 15)

    def read_bounds(self, fl, fh, nm):
        """A bounds record names one symbol of an alphabet whose other entries it does not carry: 1 if the value lies in that symbol's interval (the
        spec's `cur` of the symbol and of the one before it), which it then takes like read_symbol; -1 if not."""
        prev = self.rng if fl >= 32768 else ((self.rng >> 8) * (fl >> 6) >> 1) + 4 * (nm + 1)
        cur = ((self.rng >> 8) * (fh >> 6) >> 1) + 4 * nm
        if not cur <= self.val < prev:
            return -1
        self._renormalize(prev, cur)
        return 1


def record_value(rec):
    if rec >> 30 == 0 and rec & 0x20000000:
        return 1
    if rec >> 30 == 0:
        return (rec >> 16) & 15
    return 0 if rec == rec_bit(0) else 1


def decode_check(records, data, cdf0):
    """The spec decoder recovers every record's value from `data`."""
    dec = SpecDecoder(data, cdf0)
    for i, rec in enumerate(records):
        got = dec.read_record(rec)
        if got != record_value(rec):
            return 'record %d (%08x): decoded %d' % (i, rec, got)
    return None


# ---------------------------------------------------------------- the product's default table
def _parse_tables():
    src = open(os.path.join(ROOT, 'cavif_rs_amd', 'csrc', 'av1_tables.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (CDF_\w+) (\d+)', src)}
    body = src[src.index('av1_default_cdfs[4 * CDF_TOTAL] = {'):]
    body = body[body.index('{') + 1:body.index('};')]
    vals = [int(v) for v in body.replace('\n', ' ').split(',') if v.strip()]
    assert len(vals) == 4 * defs['CDF_TOTAL']
    return defs, vals


DEFS, _DEFAULTS = _parse_tables()
CDF_TOTAL = DEFS['CDF_TOTAL']
NCDF = CDF_TOTAL + 8                              # + the switchable restoration_type row behind the tables (tile_entropy.h CDF_LR_SWITCHABLE)


def default_table(qctx=0):
    t = _DEFAULTS[qctx * CDF_TOTAL:(qctx + 1) * CDF_TOTAL] + [32768 - 9413, 32768 - 22581, 0, 0, 0, 0, 0, 0]
    assert len(t) == NCDF
    return t


def _rows():
    D = DEFS
    # (offset, stride, rows, alphabet size): host_av1.h MI_COST_ROWS, the rows that carry symbol probabilities, + the restoration row
    spec = [('CDF_KF_Y', 25, 13), ('CDF_ANGLE', 8, 7), ('CDF_UV_NOCFL', 13, 13), ('CDF_UV_CFL', 13, 14), ('CDF_SKIP', 3, 2), ('CDF_SEG_ID', 3, 8),
            ('CDF_INTRA_TX1', 26, 7), ('CDF_INTRA_TX2', 39, 5), ('CDF_CFL_SIGN', 1, 8), ('CDF_CFL_ALPHA', 6, 16), ('CDF_TXB_SKIP', 65, 2),
            ('CDF_EOB_EXTRA', 90, 2), ('CDF_DC_SIGN', 6, 2), ('CDF_COEFF_BR', 210, 4), ('CDF_COEFF_BASE', 420, 4), ('CDF_COEFF_BASE_EOB', 40, 3),
            ('CDF_EOB_PT_16', 4, 5), ('CDF_EOB_PT_32', 4, 6), ('CDF_EOB_PT_64', 4, 7), ('CDF_EOB_PT_128', 4, 8), ('CDF_EOB_PT_256', 4, 9),
            ('CDF_EOB_PT_512', 4, 10), ('CDF_EOB_PT_1024', 4, 11)]
    rows = []
    for name, n, ns in spec:
        rows += [(D[name] + i * D[name + '_STRIDE'], ns) for i in range(n)]
    P, PS = D['CDF_PARTITION'], D['CDF_PARTITION_STRIDE']
    rows += [(P + i * PS, 4) for i in range(4)] + [(P + i * PS, 10) for i in range(4, 16)]
    rows += [(D['CDF_TX_SIZE'] + i * D['CDF_TX_SIZE_STRIDE'], 2 if i < 3 else 3) for i in range(12)]
    rows.append((CDF_TOTAL, 3))
    return rows


ROWS = _rows()                                     # every (offset, alphabet size) of the real table
PEDGE_ROWS = [DEFS['CDF_PARTITION'] + i * DEFS['CDF_PARTITION_STRIDE'] for i in range(4, 16)]   # 16x16 ... 64x64 nodes: the frame-edge bools (mi counts are even)


def row_owner(row, na):
    """tile_entropy.h k4_row_owner<2 / 4>."""
    return (row // 5 + row // 210) & (na - 1)


# ---------------------------------------------------------------- streams
class Stream:
    """records + how they are split into the kernel's record buffers (buffer sizes), the initial table, and whether the spec decoder can read it back
    (a symbol s > 0 after entries of 32768 is coded by the encoders' first-symbol branch, which no decoder inverts)."""
    def __init__(self, name, records, splits=None, cdf=None, decodable=True):
        self.name, self.records = name, list(records)
        self.splits = list(splits) if splits is not None else _chunks(len(self.records), 700)
        assert sum(self.splits) == len(self.records)
        self.cdf = list(cdf) if cdf is not None else default_table()
        assert len(self.cdf) == NCDF
        self.decodable = decodable
        self.props = {}                              # what the generator proved the stream reaches
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = encode(self.records, self.cdf)
        return self._ref


def _chunks(n, size):
    return [size] * (n // size) + ([n % size] if n % size else []) if n else [0]


def _decode_records(target, cdf, schedule):
    """Decoder-driven: the records whose values the spec decoder reads from `target` under `schedule` (a callable i -> record with a dummy value), as many
    as it takes to read past the target's end."""
    dec = SpecDecoder(target, cdf)
    out, i = [], 0
    while dec.consumed < 8 * len(target):
        rec = schedule(i)
        v = dec.read_record(rec)
        if rec >> 30 == 0 and not rec & 0x20000000:
            rec = (rec & ~(15 << 16)) | (v << 16)
        elif rec >> 30 == 1:
            rec = rec_bit(v)
        else:
            assert v == 1, 'a partition edge always splits'
        out.append(rec)
        i += 1
    return out


def _runs(data, byte):
    """(start, length) of every run of `byte`."""
    res, i = [], 0
    while i < len(data):
        if data[i] == byte:
            j = i
            while j < len(data) and data[j] == byte:
                j += 1
            res.append((i, j - i))
            i = j
        else:
            i += 1
    return res


def byte_target_streams():
    out = []
    rnd = random.Random(1001)
    bits = lambda i: rec_bit(0)
    skip_rows = [DEFS['CDF_SKIP'] + k * DEFS['CDF_SKIP_STRIDE'] for k in range(3)]
    base_rows = [DEFS['CDF_COEFF_BASE'] + k * DEFS['CDF_COEFF_BASE_STRIDE'] for k in (21, 22, 63, 64)]
    mixed = lambda i: rec_sym(base_rows[i % 4], 0, 4) if i % 3 else (rec_bit(0) if i % 2 else rec_sym(skip_rows[i % 3], 0, 2))
    for byte in (0xFF, 0x00):
        for k, run in enumerate((1, 63, 64, 65, 127, 128, 255, 256, 257, 600)):
            start = 64 * (1 + k % 3) - run // 2 - 1 if run >= 2 else 64 * (1 + k % 3) - 1   # straddling a 64-byte boundary
            lead = bytes(rnd.randrange(1, 255) for _ in range(max(start, 3)))
            tail = bytes(rnd.randrange(1, 255) for _ in range(12))
            target = lead + bytes([byte]) * run + tail
            sched = mixed if k % 2 else bits
            recs = _decode_records(target, default_table(), sched)
            s = Stream('bytes_%02x_run%d' % (byte, run), recs, splits=_chunks(len(recs), 500 + 37 * k))
            got = s.ref.data
            assert got[:len(lead) + run] == target[:len(lead) + run], s.name
            s.props['run'] = (byte, len(lead), run)
            if byte == 0 and run >= 65:                     # the units under the run are 0xFF and a carry comes up through them (kernel_units)
                chain = max([c[1] for c in carry_chains(kernel_units(s.ref.steps, s.ref.tbits))], default=0)
                assert chain >= 0.9 * run - 5, (s.name, chain)
                s.props['chain'] = chain
            out.append(s)
    # the carry that travels: top-heavy symbols (small deltas summed over and over) behind a run of 0x00 in the target: the units hold 0xFF, the carry comes from below
    for run, k in ((70, 0), (130, 1)):
        lead = bytes(rnd.randrange(1, 255) for _ in range(90 + 17 * k))
        target = lead + b'\x00' * run + bytes(rnd.randrange(1, 255) for _ in range(12))
        cdf = default_table()
        row = DEFS['CDF_COEFF_BASE'] + 30 * DEFS['CDF_COEFF_BASE_STRIDE']
        cdf[row:row + 5] = [32700, 32650, 32600, 0, 32]      # symbol 3 (the last) almost certain: every step adds nearly the whole range
        recs = _decode_records(target, cdf, lambda i: rec_sym(row, 0, 4))
        s = Stream('carry_chain_%d' % run, recs, cdf=cdf, splits=_chunks(len(recs), 300 + 64 * k))
        chain = max([c[1] for c in carry_chains(kernel_units(s.ref.steps, s.ref.tbits))], default=0)
        assert chain >= run - 4, (s.name, chain)
        s.props['chain'] = chain
        out.append(s)
    return out


def extreme_streams():
    out = []
    rnd = random.Random(2002)
    # 64-symbol chunks at minimum probability: every symbol moves the window 15 bits
    row = DEFS['CDF_COEFF_BASE'] + 7 * DEFS['CDF_COEFF_BASE_STRIDE']
    cdf = default_table(); cdf[row:row + 5] = [32767, 32766, 32765, 0, 32]       # symbols 0, 1, 2 (nearly) impossible; counter saturated, adapting slowly
    recs = [rec_sym(row, rnd.choice((1, 2)), 4) for _ in range(64 * 9)]
    out.append(Stream('min_prob_chunks', recs, cdf=cdf, splits=[64 * 4, 64 * 5]))
    recs = [rec_bounds(0, 0, 15) for _ in range(64 * 8)]                           # bounds records: a zero-probability symbol of 16, the range left at 4
    out.append(Stream('min_prob_bounds', recs, splits=[64, 64 * 3, 64 * 4]))
    # long runs of the most probable first symbol (d = 0, delta = 0), then a high-probability non-first symbol (large delta at d = 0)
    cdf = default_table(); cdf[row:row + 5] = [300, 200, 100, 0, 32]
    recs = [rec_sym(row, 0, 4) for _ in range(3000)] + [rec_bounds(2, 1, 0)] + [rec_sym(row, 0, 4) for _ in range(500)]
    out.append(Stream('mps_first_runs', recs, cdf=cdf))
    cdf = default_table(); cdf[row:row + 5] = [20000, 300, 200, 0, 0]             # symbol 1 at 0.6: a delta of ~0.39 of the range, the window mostly still
    recs = [rec_sym(row, 1 if rnd.random() < 0.9 else rnd.choice((0, 2, 3)), 4) for _ in range(2000)]
    recs += [rec_bounds(400, 0, 0) if rnd.random() < 0.8 else rec_bit(rnd.randrange(2)) for _ in range(1500)]   # the last symbol at 0.78: delta ~0.22 of the range
    out.append(Stream('mps_non_first', recs, cdf=cdf))
    # CDF extremes: entries of 32768 / 0, equal neighbours (zero-probability symbols), every alphabet size 2 .. 16 (rows laid into the free tail of the table)
    cdf = default_table()
    rows = []
    pos = DEFS['CDF_EOB_PT_16']
    for ns in range(2, 17):
        assert pos + ns < CDF_TOTAL
        vals = sorted((rnd.randrange(0, 32768) for _ in range(ns - 1)), reverse=True)
        if ns % 3 == 0:
            vals[0] = vals[1] if ns > 2 else vals[0]                               # equal neighbours: symbol 1 has zero probability
        if ns % 4 == 0:
            vals[-1] = 0                                                           # symbol ns - 2 takes what is left down to 0, the last one nothing
        cdf[pos:pos + ns + 1] = vals + [0, rnd.choice((0, 14, 15, 16, 30, 31, 32))]
        rows.append((pos, ns))
        pos += ns + 1
    recs = []
    for i in range(4000):
        off, ns = rows[i % len(rows)] if i % 7 else rnd.choice(rows)
        recs.append(rec_sym(off, rnd.randrange(ns), ns))
    out.append(Stream('alphabets_2_to_16', recs, cdf=cdf))
    # entries of 32768: a row whose symbol 0 is impossible; a symbol s > 0 behind it takes the first-symbol branch (fl >> 6 = 512) of every encoder
    cdf = default_table()
    pos = DEFS['CDF_EOB_PT_16']
    cdf[pos:pos + 6] = [32768, 20000, 9000, 9000, 0, 0]
    recs = [rec_sym(pos, rnd.choice((1, 1, 2, 3, 4)), 5) for _ in range(600)] + [rec_bit(rnd.randrange(2)) for _ in range(50)]
    out.append(Stream('entry_32768_first_symbol_branch', recs, cdf=cdf, decodable=False))
    # the adaptation counter through 15 / 16, 31 / 32 and saturation, on alphabets of 2, 3, 4 and 8+ (three rate classes)
    recs = []
    for off, ns in [(DEFS['CDF_SKIP'], 2), (DEFS['CDF_COEFF_BASE_EOB'], 3), (DEFS['CDF_COEFF_BASE'], 4), (DEFS['CDF_KF_Y'], 13)]:
        recs += [rec_sym(off, rnd.randrange(ns), ns) for _ in range(40)]
    s = Stream('counter_15_31_32', recs, splits=[15, 1, 15, 1, 8, 120])
    out.append(s)
    return out


def split_streams():
    out = []
    rnd = random.Random(3003)
    mk = lambda n: [rnd.choice((rec_sym(*_sym_of(rnd)), rec_bit(rnd.randrange(2)))) for _ in range(n)]
    out.append(Stream('empty_tile', [], splits=[]))
    out.append(Stream('empty_buffers', [], splits=[0, 0, 0]))
    for n in (1, 63, 64, 65):
        out.append(Stream('one_buffer_%d' % n, mk(n), splits=[n]))
    recs = mk(300)
    out.append(Stream('buffers_0_1_63_64_65', recs[:193], splits=[0, 1, 63, 0, 64, 65]))
    # the tile's end at every bit phase of T and chunk fills 1, 2, 16, 17, 63, 64 of the last 64-symbol chunk
    seen = set()
    fills = (1, 2, 16, 17, 63, 64)
    i = 0
    while len(seen) < 8 * len(fills):
        assert i < 5000
        fill = fills[i % len(fills)]
        n = 64 * (i % 5) + fill
        recs = mk(n)
        ph = encode(recs, default_table()).tbits & 7
        if (ph, fill) not in seen:
            seen.add((ph, fill))
            out.append(Stream('end_phase%d_fill%d' % (ph, fill), recs, splits=_chunks(n, 64 * (1 + i % 3))))
        i += 1
    return out


def _sym_of(rnd):
    off, ns = rnd.choice(ROWS)
    return off, rnd.randrange(ns), ns


def row_streams():
    out = []
    rnd = random.Random(4004)
    # every row of the real table at least once (so both k4_row_owner<2> and <4> give every adapter rows), a change of row on every record
    rows = [r for r in ROWS]
    rnd.shuffle(rows)
    recs = [rec_sym(off, rnd.randrange(ns), ns) for off, ns in rows]
    out.append(Stream('every_row_once', recs))
    # runs of hundreds of records on one row (the adapter keeps it in a register) interleaved with a change of row on every record, partition edges between
    recs = []
    for k in range(8):
        off, ns = rnd.choice(ROWS)
        recs += [rec_sym(off, rnd.randrange(ns) if k % 2 else 0, ns) for _ in range(rnd.choice((200, 300, 450)))]
        for _ in range(150):
            off, ns = rnd.choice(ROWS)
            recs.append(rec_sym(off, rnd.randrange(ns), ns))
            if rnd.random() < 0.15:
                recs.append(rec_pedge(rnd.choice(PEDGE_ROWS), rnd.randrange(2)))
    out.append(Stream('runs_and_row_changes', recs))
    # partition-edge bools read from rows as they stand: symbols on the same partition rows around them, has_cols 0 and 1
    recs = []
    for _ in range(1500):
        r = rnd.choice(PEDGE_ROWS)
        recs.append(rec_pedge(r, rnd.randrange(2)) if rnd.random() < 0.4 else rec_sym(r, rnd.randrange(10), 10))
    out.append(Stream('partition_edges', recs))
    return out


def random_streams(n=12, seed=5005):
    out = []
    rnd = random.Random(seed)
    for k in range(n):
        recs = []
        for _ in range(rnd.choice((50, 400, 1500, 4000))):
            x = rnd.random()
            if x < 0.6:
                recs.append(rec_sym(*_sym_of(rnd)))
            elif x < 0.9:
                recs.append(rec_bit(rnd.randrange(2)))
            else:
                recs.append(rec_pedge(rnd.choice(PEDGE_ROWS), rnd.randrange(2)))
        splits, left = [], len(recs)
        while left:
            c = min(left, rnd.choice((0, 1, 64, 65, 200, 777)))
            splits.append(c)
            left -= c
        out.append(Stream('random_%02d' % k, recs, splits=splits or [0]))
    return out


def all_streams():
    return byte_target_streams() + extreme_streams() + split_streams() + row_streams() + random_streams()
