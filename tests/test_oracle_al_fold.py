"""CPU pins for the aligned fused kernel's chained full-frame CRC fold
(rs_encode_frame_al_k): the x^(8*13312) byte-sliced table and the four-pass
Horner chain with one position fold per lane, both against the oracle."""
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


def _raw(oracle, chunk):
    """table update from state 0, no complements"""
    return 0xFFFFFFFF ^ oracle.crc32(chunk, crc=0xFFFFFFFF)


T13K = _shift_table(13312)
T1K = _shift_table(1024)


def test_shift13k_table_is_a_13312_byte_zero_extension(oracle):
    # 13312 = 2^13 + 2^12 + 2^10, the decomposition the host builder uses
    assert _x8n(13312) == _mulmod(_mulmod(_x8n(8192), _x8n(4096)), _x8n(1024))
    for j in range(4):
        for b in range(256):
            assert T13K[j][b] == oracle.crc32_shift(b << (8 * j), 13312)
    rng = np.random.default_rng(13312)
    for v in rng.integers(0, 1 << 32, 64, dtype=np.uint64):
        assert _shift(int(v), T13K) == oracle.crc32_shift(int(v), 13312)
    # against a real CRC: raw(piece || 13312 zeros) == shift(raw(piece))
    piece = rng.integers(0, 256, 16, dtype=np.uint8)
    ext = np.concatenate([piece, np.zeros(13312, np.uint8)])
    assert _shift(_raw(oracle, piece), T13K) == _raw(oracle, ext)


def test_chained_four_pass_fold_is_the_frame_crc(oracle):
    """The kernel's full-frame form: the 65536-B image (header slot zeroed)
    is 4096 chunks; lane tid of wave w chains chunks 1024h + 256w + 64i +
    lane over passes h and pieces i (1024 B steps inside a pass, 13312 B
    from piece 3 to the next pass's piece 0) and folds once by the suffix
    after its last piece."""
    rng = np.random.default_rng(65532)
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
                    _raw(oracle, img[16 * q:16 * q + 16])
        fold ^= oracle.crc32_shift(t, 16384 - 16 * (ql0 + 193))
    crc = 0xFFFFFFFF ^ oracle.crc32_shift(0xFFFFFFFF, 65532) ^ fold
    assert crc == oracle.crc32(buf)
