"""CPU pins for the aligned fused kernel's 12-gather piece form (crc12u_reg
in rs_encode_frame_al_k): u(piece) is the raw CRC of the piece short of its
last x^32, in the two-level form (8 gathers, then 4, the fourth dword raw)
and in the one-level slice-by-12 form; chained as before and folded by the
suffix operator plus 4 bytes it gives the frame CRC.  All against the
oracle."""
import numpy as np

POLY = 0xEDB88320


def _mulmod(a, b):
    """reflected-domain carry-less multiply mod P, as the host table builder"""
    prod = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            prod ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return prod


def _x8n(nbytes):
    op, p = 0x80000000, 0x00800000  # identity, x^8
    while nbytes:
        if nbytes & 1:
            op = _mulmod(op, p)
        p = _mulmod(p, p)
        nbytes >>= 1
    return op


def _shift_table(nbytes):
    x = _x8n(nbytes)
    return [[_mulmod(x, b << (8 * j)) for b in range(256)] for j in range(4)]


def _shift(c, tab):
    return (tab[0][c & 0xFF] ^ tab[1][(c >> 8) & 0xFF] ^
            tab[2][(c >> 16) & 0xFF] ^ tab[3][c >> 24])


def _slice_tables(n):
    """the host builder's slice-by-n construction; tab[0] is the byte table"""
    t0 = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        t0.append(c)
    tab = [t0]
    for _ in range(1, n):
        tab.append([t0[v & 0xFF] ^ (v >> 8) for v in tab[-1]])
    return tab


TAB = _slice_tables(12)
T13K = _shift_table(13312)
T1K = _shift_table(1024)


def _bytes4(w, hi):
    """the four gathers of one dword over tab[hi], tab[hi-1], ..."""
    return (TAB[hi][w & 0xFF] ^ TAB[hi - 1][(w >> 8) & 0xFF] ^
            TAB[hi - 2][(w >> 16) & 0xFF] ^ TAB[hi - 3][w >> 24])


def _dwords(piece):
    return [int(x) for x in np.frombuffer(bytes(piece), dtype="<u4")]


def _u_two_level(piece):
    d0, d1, d2, d3 = _dwords(piece)
    c = _bytes4(d0, 7) ^ _bytes4(d1, 3)
    return _bytes4(c ^ d2, 3) ^ d3


def _u_one_level(piece):
    d0, d1, d2, d3 = _dwords(piece)
    return _bytes4(d0, 11) ^ _bytes4(d1, 7) ^ _bytes4(d2, 3) ^ d3


def _raw(oracle, chunk):
    """table update from state 0, no complements"""
    return 0xFFFFFFFF ^ oracle.crc32(chunk, crc=0xFFFFFFFF)


def _pieces():
    rng = np.random.default_rng(12)
    out = [p for p in rng.integers(0, 256, (256, 16), dtype=np.uint8)]
    out.append(np.zeros(16, np.uint8))
    for pos in (0, 7, 8, 11, 12, 15):
        for val in (0x01, 0x80, 0xA5):
            p = np.zeros(16, np.uint8)
            p[pos] = val
            out.append(p)
    return out


def test_piece_u_times_x32_is_the_raw_crc(oracle):
    for p in _pieces():
        u = _u_two_level(p)
        assert u == _u_one_level(p), bytes(p).hex()
        assert oracle.crc32_shift(u, 4) == _raw(oracle, p), bytes(p).hex()


def test_chained_u_pieces_fold_to_the_frame_crc(oracle):
    """test_oracle_al_fold's four-pass chain with u pieces: every piece is
    short by x^32, the shifts are linear, so the whole chain is short by
    x^32 and the lane's operator takes 4 bytes more."""
    rng = np.random.default_rng(65532 + 12)
    buf = rng.integers(0, 256, 65532, dtype=np.uint8)
    img = np.concatenate([np.zeros(4, np.uint8), buf])
    fold = 0
    for tid in range(256):
        ql0 = (tid >> 6) * 256 + (tid & 63)
        t = 0
        for h in range(4):
            for i in range(4):
                q = 1024 * h + ql0 + 64 * i
                t = _shift(t, T13K if i == 0 else T1K) ^ \
                    _u_two_level(img[16 * q:16 * q + 16])
        fold ^= oracle.crc32_shift(t, 16384 - 16 * (ql0 + 193) + 4)
    crc = 0xFFFFFFFF ^ oracle.crc32_shift(0xFFFFFFFF, 65532) ^ fold
    assert crc == oracle.crc32(buf)
