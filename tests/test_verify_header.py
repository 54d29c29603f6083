"""Header classification of stored fragments (frag_check.hpp through
ecamd_classify_header; the batch verify kernel runs the same function on the
device): headers from the oracle's encode, mutated one field at a time,
against the literal expectation and against the pure-Python restatement
below of the semantics in include/erasurecode_amd.h (ecamd_verify_batch).
The reference's checks: is_invalid_fragment_header / is_invalid_fragment, as
pinned by test/test_pyeclib_api.py:574-648 and :877-903.  CPU only."""
import pytest

from pyeclib_amd import _native

HDR = 80
MAGIC = 0xB0C5ECC
RS_VAND = 6  # the id liberasurecode_rs_vand and amd_rs_vand write (byte 54)
OK, BAD_HEADER, BAD_CHKSUM = 0, 1, 2


def _u32(b, at):
    return int.from_bytes(b[at:at + 4], "little")


def classify_header(O, hdr, wire_id, slot, bs, obj_len):
    """0 sound, 1 bad header, 2 sound with chksum_mismatch set."""
    ver, magic = _u32(hdr, 63), _u32(hdr, 59)
    if ver == 0:
        return BAD_HEADER
    if ver >= 0x010200:
        if magic != MAGIC:
            return BAD_HEADER
        if _u32(hdr, 67) not in (O.crc32(bytes(hdr[:59])), O.crc32_legacy(bytes(hdr[:59]))):
            return BAD_HEADER
    if ver > 0x010800 or magic != MAGIC:
        return BAD_HEADER
    if hdr[54] != wire_id or not 1 <= hdr[20] <= 3:
        return BAD_HEADER
    if _u32(hdr, 0) != slot or _u32(hdr, 4) != bs or \
            int.from_bytes(hdr[12:20], "little") != obj_len:
        return BAD_HEADER
    return BAD_CHKSUM if hdr[53] == 1 else OK


def classify_fragment(O, frag, wire_id, slot, bs, obj_len):
    """The whole classification of one slot's bytes: 0, 1 (bad_header) or
    2 (bad_chksum).  Only frag[:80 + bs] is looked at."""
    v = classify_header(O, frag[:HDR], wire_id, slot, bs, obj_len)
    if v != OK or frag[20] != 2:
        return v
    payload = bytes(frag[HDR:HDR + bs])
    return OK if _u32(frag, 21) in (O.crc32(payload), O.crc32_legacy(payload)) else BAD_CHKSUM


def remeta(O, h):
    """Recompute the metadata checksum (zlib's CRC of bytes 0..58 at 67)."""
    h[67:71] = O.crc32(bytes(h[:59])).to_bytes(4, "little")
    return h


def _set(at, value, width=4, fix=True):
    def mutate(O, h):
        h[at:at + width] = value.to_bytes(width, "little")
        return remeta(O, h) if fix else h
    return mutate


def _add(at, delta, width=4):
    def mutate(O, h):
        v = (int.from_bytes(h[at:at + width], "little") + delta) % (1 << (8 * width))
        h[at:at + width] = v.to_bytes(width, "little")
        return remeta(O, h)
    return mutate


def _flip(at, bit):
    def mutate(O, h):
        h[at] ^= 1 << bit
        return h
    return mutate


def _old_version(wrong_magic):
    def mutate(O, h):
        h[63:67] = (0x010100).to_bytes(4, "little")
        h[67] ^= 0x5A  # a wrong metadata checksum: not looked at below 1.2.0
        if wrong_magic:
            h[59] ^= 1
        return h
    return mutate


# (name, mutation of a sound header, expected class); shared with the GPU test
MUTATIONS = [
    ("sound", lambda O, h: h, OK),
    ("magic", _flip(59, 3), BAD_HEADER),
    ("meta_chksum", _flip(69, 0), BAD_HEADER),
    ("legacy_meta_chksum", lambda O, h: bytearray(O.legacy_headers(bytes(h))), OK),
    ("version_0", _set(63, 0, fix=False), BAD_HEADER),
    ("version_1_1_0_wrong_meta", _old_version(False), OK),
    ("version_1_1_0_wrong_magic", _old_version(True), BAD_HEADER),
    ("version_1_9_0", _set(63, 0x010900, fix=False), BAD_HEADER),
    ("backend_id_4", _set(54, 4, 1), BAD_HEADER),
    ("chksum_type_0", _set(20, 0, 1), BAD_HEADER),
    ("chksum_type_4", _set(20, 4, 1), BAD_HEADER),
    ("chksum_mismatch", _set(53, 1, 1), BAD_CHKSUM),
    ("idx_plus_1", _add(0, 1), BAD_HEADER),
    ("idx_minus_1", _add(0, -1), BAD_HEADER),
    ("size_plus_1", _add(4, 1), BAD_HEADER),
    ("size_minus_1", _add(4, -1), BAD_HEADER),
    ("orig_plus_1", _add(12, 1, 8), BAD_HEADER),
    ("orig_minus_1", _add(12, -1, 8), BAD_HEADER),
] + [(f"bit_byte_{at}", _flip(at, at % 8), BAD_HEADER) for at in range(59)]

K, M, OBJ_LEN = 4, 2, 1000


@pytest.fixture(scope="module")
def stripe(oracle):
    data = bytes((7 * i + 3) & 0xFF for i in range(OBJ_LEN))
    return oracle.encode(K, M, data, oracle.CHKSUM_CRC32)


def native(hdr, slot, bs, obj_len, backend=RS_VAND):
    return _native.lib.ecamd_classify_header(bytes(hdr), backend, slot, bs, obj_len)


@pytest.mark.parametrize("slot", [1, 5])
@pytest.mark.parametrize("name,mutate,want", MUTATIONS, ids=[c[0] for c in MUTATIONS])
def test_classify_header(oracle, stripe, slot, name, mutate, want):
    bs = oracle.blocksize(K, OBJ_LEN)
    h = bytearray(mutate(oracle, bytearray(stripe[slot])))[:HDR]
    assert classify_header(oracle, h, RS_VAND, slot, bs, OBJ_LEN) == want
    assert native(h, slot, bs, OBJ_LEN) == want
    # amd_rs_vand writes (and expects) liberasurecode_rs_vand's id
    assert native(h, slot, bs, OBJ_LEN, backend=11) == want


def test_classify_header_layout_arguments(oracle, stripe):
    """A sound header is only sound in its own slot, for its own payload
    size and object length, on an instance of its own backend."""
    bs = oracle.blocksize(K, OBJ_LEN)
    h = stripe[2][:HDR]
    assert native(h, 2, bs, OBJ_LEN) == OK
    assert native(h, 3, bs, OBJ_LEN) == BAD_HEADER
    assert native(h, 2, bs + 2, OBJ_LEN) == BAD_HEADER
    assert native(h, 2, bs, OBJ_LEN - 1) == BAD_HEADER
    assert native(h, 2, bs + (1 << 32), OBJ_LEN) == BAD_HEADER
    assert native(h, 2, bs, OBJ_LEN, backend=4) == BAD_HEADER  # isa_l_rs_vand instance
    assert native(h, 2, bs, OBJ_LEN, backend=99) == -_native.EINVALIDPARAMS
    none = oracle.encode(K, M, b"x" * OBJ_LEN)[2][:HDR]  # chksum_type NONE
    assert none[20] == 1 and native(none, 2, bs, OBJ_LEN) == OK


def test_restatement_payload_checksum(oracle, stripe):
    """The restatement's payload half (what the GPU tests expect)."""
    bs = oracle.blocksize(K, OBJ_LEN)
    f = bytearray(stripe[0])
    assert classify_fragment(oracle, f, RS_VAND, 0, bs, OBJ_LEN) == OK
    assert classify_fragment(oracle, bytearray(oracle.legacy_headers(bytes(f))), RS_VAND, 0, bs,
                             OBJ_LEN) == OK
    f[HDR + bs - 1] ^= 0x10
    assert classify_fragment(oracle, f, RS_VAND, 0, bs, OBJ_LEN) == BAD_CHKSUM
