"""Batch verify on the GPU (BatchCodec.verify / usable_masks / verify_report,
ecamd_verify_batch, ec_verify.hip): fragment headers and payload CRC-32
checked where the stripes live.  Every expected mask comes from the
pure-Python restatement in tests/test_verify_header.py (classify_fragment, on
the oracle's crc32 / crc32_legacy), never from the library under test.  Every
corruption is a byte inside the test's own stripe buffer.

The reference's counterparts: ECDriver.decode(force_metadata_checks=True),
get_metadata's chksum_mismatch and verify_stripe_metadata
(test/test_pyeclib_api.py:574-648, :877-903)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_verify_header import (BAD_CHKSUM, BAD_HEADER, MUTATIONS, OK,  # noqa: E402
                                classify_fragment, remeta)

pytestmark = pytest.mark.gpu

HDR = 80
WIRE = {"amd_rs_vand": 6, "liberasurecode_rs_vand": 6, "isa_l_rs_vand": 4, "isa_l_rs_cauchy": 7}
RUN = 16  # ec_verify.hpp kVerifyRunChunks: 1 KiB chunks per work item


def r16(x):
    return (x + 15) // 16 * 16


def new_buffer(batch, gpu, n_obj, k, m, bs, packed):
    """A zeroed (n_obj, k+m, frag_stride) stripe buffer: the library's
    (128-byte-aligned payloads) or packed (payloads 16- but not 128-byte
    aligned)."""
    import torch
    if not packed:
        return batch.stripe_buffer(n_obj, k, m, bs, device=gpu)
    fs = r16(HDR + r16(bs))
    flat = torch.zeros(n_obj * (k + m) * fs, dtype=torch.uint8, device=gpu)
    assert flat.data_ptr() % 128 == 0
    return flat.view(n_obj, k + m, fs)


def encode_stripes(codec, gpu, obj_len, n_obj, packed=False, seed=1):
    """Objects (host) and their full stripes (device), encode still queued."""
    import torch
    from pyeclib_amd import batch
    bs = codec.blocksize(obj_len)
    host = torch.from_numpy(np.random.default_rng(seed + obj_len).integers(
        0, 256, (n_obj, r16(obj_len)), dtype=np.uint8))
    frags = new_buffer(batch, gpu, n_obj, codec.k, codec.m, bs, packed)
    codec.encode(host.to(gpu), obj_len, parity=frags[:, codec.k:], data=frags[:, :codec.k])
    return host, frags, bs


def expected(oracle, stripes, ec_type, bs, obj_len, present=None):
    """[[bad_header, bad_chksum]] per object from the restatement over the
    host copy `stripes` (n_obj, k+m, frag_stride)."""
    out = []
    for o in range(stripes.shape[0]):
        bh = bc = 0
        for i in range(stripes.shape[1]):
            if present is not None and not present[o] >> i & 1:
                continue
            v = classify_fragment(oracle, stripes[o, i].tobytes(), WIRE[ec_type], i, bs, obj_len)
            bh |= (v == BAD_HEADER) << i
            bc |= (v == BAD_CHKSUM) << i
        out.append([bh, bc])
    return out


def masks_of(res):
    """Device (n_obj, 2) int32 result -> [[bad_header, bad_chksum]] unsigned."""
    return [[v & 0xFFFFFFFF for v in row] for row in res.cpu().tolist()]


def upload(batch, gpu, stripes, k, m, bs, packed=False):
    """A device stripe buffer holding the host copy `stripes`."""
    import torch
    dev = new_buffer(batch, gpu, stripes.shape[0], k, m, bs, packed)
    assert tuple(dev.shape) == stripes.shape
    dev.copy_(torch.from_numpy(stripes))
    return dev


CLEAN = [
    ("amd_rs_vand", 4, 2, 1, 3),                  # bs = 2
    ("amd_rs_vand", 4, 2, 1000, 3),               # bs = 250: no full chunk
    ("amd_rs_vand", 4, 2, 4096, 3),               # bs = 1024 exactly
    ("amd_rs_vand", 4, 2, 4104, 3),               # bs = 1026
    ("isa_l_rs_vand", 8, 4, 65537, 3),            # bs = 8193: odd, tail not a multiple of 16
    ("isa_l_rs_cauchy", 12, 4, 300001, 2),
    ("liberasurecode_rs_vand", 4, 2, 20001, 2),
    ("amd_rs_vand", 10, 4, 4 << 20, 1),           # one object must still be split across blocks
    ("amd_rs_vand", 10, 4, 4 << 20, 5),
    ("amd_rs_vand", 6, 6, 300001, 4),
    ("amd_rs_vand", 4, 2, 4 * (RUN * 1024 + 2), 2),  # bs = run length x 1024 + 2
    ("amd_rs_vand", 4, 2, 4 * (RUN * 1024 - 2), 2),  # ... and - 2
]


@pytest.mark.parametrize("packed", [False, True], ids=["aligned128", "packed16"])
@pytest.mark.parametrize("ec_type,k,m,obj_len,n_obj", CLEAN)
def test_clean_stripes_report_zero(oracle, gpu, ec_type, k, m, obj_len, n_obj, packed):
    """inline_crc32 full stripes verified on the same stream with no
    synchronise in between (so verify is ordered behind the finishing pass):
    nothing is reported, and a flipped payload bit in the last fragment's
    last byte then is."""
    import torch
    from pyeclib_amd import batch
    codec = batch.BatchCodec(k, m, inline_crc32=True, ec_type=ec_type)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj, packed)
    if ec_type == "amd_rs_vand" and obj_len == 4 * (RUN * 1024 + 2):
        assert bs == RUN * 1024 + 2
    assert (frags.data_ptr() + HDR) % 128 == (80 if packed else 0)
    res = codec.verify(frags, obj_len)
    torch.cuda.synchronize()
    host = frags.cpu().numpy()
    want = expected(oracle, host, ec_type, bs, obj_len)
    assert want == [[0, 0]] * n_obj
    assert masks_of(res) == want
    frags[n_obj - 1, k + m - 1, HDR + bs - 1] ^= 0x80
    assert masks_of(codec.verify(frags, obj_len))[n_obj - 1] == [0, 1 << (k + m - 1)]


def test_payload_bit_flips_found_where_they_are(oracle, gpu):
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 10, 4, 1 << 20, 6
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    assert frags.shape[2] > HDR + bs  # the slot has padding past the payload
    flips = [(0, 0, 0), (1, 3, 1023), (2, 13, 1024), (3, 7, bs // 2), (4, 10, bs - 17),
             (5, 9, bs - 1), (0, 12, bs - 1)]
    for n, (o, i, at) in enumerate(flips):
        frags[o, i, HDR + at] ^= 1 << (n % 8)
    frags[1, 5, HDR + bs] ^= 0x40  # padding: part of nothing
    res = codec.verify(frags, obj_len)
    torch.cuda.synchronize()
    want = [[0, 0] for _ in range(n_obj)]
    for o, i, _ in flips:
        want[o][1] |= 1 << i
    assert expected(oracle, frags.cpu().numpy(), "amd_rs_vand", bs, obj_len) == want
    assert masks_of(res) == want


@pytest.mark.parametrize("packed", [False, True], ids=["aligned128", "packed16"])
def test_header_cases_on_device(oracle, gpu, packed):
    """The CPU test's header mutations, one per (object, fragment), and two
    fragments swapped between slots (both bad by idx)."""
    import torch
    from pyeclib_amd import batch
    k, m, obj_len = 4, 2, 1000
    n_obj = (len(MUTATIONS) + k + m - 1) // (k + m) + 1
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj, packed)
    torch.cuda.synchronize()
    host = frags.cpu().numpy().copy()
    want = [[0, 0] for _ in range(n_obj)]
    for n, (_, mutate, cls) in enumerate(MUTATIONS):
        o, i = divmod(n, k + m)
        f = bytearray(mutate(oracle, bytearray(host[o, i, :HDR + bs].tobytes())))
        host[o, i, :HDR + bs] = np.frombuffer(bytes(f), dtype=np.uint8)
        want[o][0] |= (cls == BAD_HEADER) << i
        want[o][1] |= (cls == BAD_CHKSUM) << i
    a, b = host[n_obj - 1, 1].copy(), host[n_obj - 1, 4].copy()
    host[n_obj - 1, 1], host[n_obj - 1, 4] = b, a
    want[n_obj - 1][0] |= (1 << 1) | (1 << 4)
    assert expected(oracle, host, "amd_rs_vand", bs, obj_len) == want
    dev = upload(batch, gpu, host, k, m, bs, packed)
    assert masks_of(codec.verify(dev, obj_len)) == want


def test_both_crc_variants_accepted(oracle, gpu, monkeypatch):
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 6, 3, 20001, 4
    default = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(default, gpu, obj_len, n_obj)
    torch.cuda.synchronize()
    host = frags.cpu().numpy().copy()
    # half the fragments rewritten with liberasurecode's legacy CRCs
    for o in range(n_obj):
        for i in range(o % 2, k + m, 2):
            f = oracle.legacy_headers(host[o, i, :HDR + bs].tobytes())
            assert f[:HDR] != host[o, i, :HDR].tobytes()
            host[o, i, :HDR + bs] = np.frombuffer(f, dtype=np.uint8)
    assert expected(oracle, host, "amd_rs_vand", bs, obj_len) == [[0, 0]] * n_obj
    mixed = upload(batch, gpu, host, k, m, bs)
    assert masks_of(default.verify(mixed, obj_len)) == [[0, 0]] * n_obj
    # a legacy fragment with a payload bit flipped, next to a zlib one
    mixed[1, 1, HDR + 1500] ^= 2
    mixed[1, 2, HDR + bs - 1] ^= 2
    want = [[0, 0], [0, (1 << 1) | (1 << 2)], [0, 0], [0, 0]]
    assert expected(oracle, mixed.cpu().numpy(), "amd_rs_vand", bs, obj_len) == want
    assert masks_of(default.verify(mixed, obj_len)) == want
    # stripes written under LIBERASURECODE_WRITE_LEGACY_CRC=1
    monkeypatch.setenv("LIBERASURECODE_WRITE_LEGACY_CRC", "1")
    legacy = batch.BatchCodec(k, m, inline_crc32=True)
    _, lfrags, _ = encode_stripes(legacy, gpu, obj_len, n_obj)
    res_legacy = legacy.verify(lfrags, obj_len)
    res_default = default.verify(lfrags, obj_len)
    torch.cuda.synchronize()
    lhost = lfrags.cpu().numpy()
    payload = lhost[0, 0, HDR:HDR + bs].tobytes()
    assert int.from_bytes(lhost[0, 0, 21:25].tobytes(), "little") == oracle.crc32_legacy(payload)
    assert expected(oracle, lhost, "amd_rs_vand", bs, obj_len) == [[0, 0]] * n_obj
    assert masks_of(res_legacy) == [[0, 0]] * n_obj
    assert masks_of(res_default) == [[0, 0]] * n_obj
    # the legacy instance takes zlib fragments too, and still finds a flip
    assert masks_of(legacy.verify(frags, obj_len)) == [[0, 0]] * n_obj
    lfrags[2, 8, HDR + 7] ^= 0x20
    assert masks_of(legacy.verify(lfrags, obj_len))[2] == [0, 1 << 8]
    assert masks_of(default.verify(lfrags, obj_len))[2] == [0, 1 << 8]


def test_no_checksum_no_payload_claim(oracle, gpu):
    """Stripes of an instance without inline_crc32 (chksum_type NONE):
    payload corruption is not reported, header corruption is -- by instances
    with and without inline_crc32 alike."""
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 4, 2, 20001, 3
    plain = batch.BatchCodec(k, m)
    _, frags, bs = encode_stripes(plain, gpu, obj_len, n_obj)
    torch.cuda.synchronize()
    assert int(frags[0, 0, 20]) == 1
    frags[0, 1, HDR + 100] ^= 1
    frags[2, 5, HDR + bs - 1] ^= 1
    frags[1, 3, 5] ^= 4   # size
    frags[2, 0, 59] ^= 1  # magic
    want = [[0, 0], [1 << 3, 0], [1 << 0, 0]]
    assert expected(oracle, frags.cpu().numpy(), "amd_rs_vand", bs, obj_len) == want
    assert masks_of(plain.verify(frags, obj_len)) == want
    assert masks_of(batch.BatchCodec(k, m, inline_crc32=True).verify(frags, obj_len)) == want


def test_present_masks(oracle, gpu):
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 6, 3, 20001, 5
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    full = (1 << (k + m)) - 1
    present = [full, 0, 0b101010101, full & ~(1 << 8), 1 << 4]
    for o in range(n_obj):
        for i in range(k + m):
            if not present[o] >> i & 1:
                frags[o, i] = 0xA5  # garbage in the slots nobody asked about
    frags[2, 2, HDR + 3] ^= 1     # a selected slot that is rotten
    res = codec.verify(frags, obj_len, present)
    torch.cuda.synchronize()
    host = frags.cpu().numpy()
    want = expected(oracle, host, "amd_rs_vand", bs, obj_len, present)
    assert want == [[0, 0], [0, 0], [0, 1 << 2], [0, 0], [0, 0]]
    assert masks_of(res) == want
    # None = every slot: the garbage slots are bad headers
    want_all = expected(oracle, host, "amd_rs_vand", bs, obj_len)
    assert want_all[1] == [full, 0] and want_all[3] == [1 << 8, 0]
    assert masks_of(codec.verify(frags, obj_len)) == want_all
    assert masks_of(codec.verify(frags, obj_len, [full] * n_obj)) == want_all
    assert masks_of(codec.verify(frags, obj_len, [0xFFFFFFFF] * n_obj)) == want_all


def test_randomised_agreement(oracle, gpu):
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 6, 3, 20001, 64
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    torch.cuda.synchronize()
    host = frags.cpu().numpy().copy()
    rng = np.random.default_rng(20261019)
    touched = 0
    for o in range(n_obj):
        for i in rng.choice(k + m, size=int(rng.integers(0, 4)), replace=False):
            kind = int(rng.integers(0, 3))  # payload bit, header bit, nothing
            if kind == 0:
                host[o, i, HDR + int(rng.integers(0, bs))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                host[o, i, int(rng.integers(0, HDR))] ^= 1 << int(rng.integers(0, 8))
            touched += kind < 2
    want = expected(oracle, host, "amd_rs_vand", bs, obj_len)
    assert touched > 20 and sum(1 for w in want if w != [0, 0]) > 10
    dev = upload(batch, gpu, host, k, m, bs)
    assert masks_of(codec.verify(dev, obj_len)) == want


def test_fragments_untouched_and_non_default_stream(oracle, gpu):
    """verify only reads: the stripe buffer is byte-identical afterwards,
    padding included.  Run on a stream of the caller's, into a caller's
    result tensor."""
    import torch
    from pyeclib_amd import batch
    k, m, obj_len, n_obj = 10, 4, 300001, 3
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    frags[1, 11, HDR + bs // 3] ^= 8
    frags[2, 0, 0] ^= 1
    frags[:, :, HDR + bs:] = 0x3C
    out = torch.full((n_obj, 2), -1, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    before = frags.cpu().numpy().copy()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        res = codec.verify(frags, obj_len, out=out)
    res2 = codec.verify(frags, obj_len, stream=s)
    s.synchronize()
    assert res.data_ptr() == out.data_ptr()
    want = [[0, 0], [0, 1 << 11], [1 << 0, 0]]
    assert expected(oracle, before, "amd_rs_vand", bs, obj_len) == want
    assert masks_of(out) == want and masks_of(res2) == want
    torch.cuda.synchronize()
    assert np.array_equal(frags.cpu().numpy(), before)


def test_usable_masks_feed_decode(oracle, gpu):
    """The batch form of force_metadata_checks: usable_masks -> decode."""
    import torch
    from pyeclib_amd import batch
    from pyeclib_amd import exceptions as X
    k, m, obj_len, n_obj = 10, 4, 300001, 3
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    objs, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    full = (1 << (k + m)) - 1
    # 2 of 4 parity fragments and 1 data fragment rotten, in different ways
    frags[0, 11, HDR + 5] ^= 1
    frags[0, 13, 4] ^= 1
    frags[0, 2, HDR + bs - 1] ^= 0x80
    frags[2, 10, 59] ^= 2
    frags[2, 12, HDR + 2048] ^= 2
    frags[2, 0, HDR] ^= 2
    masks = codec.usable_masks(frags, obj_len)
    assert masks == [full & ~((1 << 11) | (1 << 13) | (1 << 2)), full,
                     full & ~((1 << 10) | (1 << 12) | (1 << 0))]
    out = torch.zeros((n_obj, objs.shape[1]), dtype=torch.uint8, device=gpu)
    codec.decode(frags, obj_len, masks, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :obj_len].cpu(), objs[:, :obj_len])
    # slots the caller already knows are gone stay out of the masks
    assert codec.usable_masks(frags, obj_len, [full & ~(1 << 5)] * n_obj) == \
        [v & ~(1 << 5) for v in masks]
    # 5 of 14 rotten: decode refuses
    frags[1, 1, HDR + 9] ^= 1
    frags[1, 4, HDR + 1024] ^= 1
    frags[1, 6, 20] ^= 1
    frags[1, 9, HDR + bs // 2] ^= 1
    frags[1, 13, 67] ^= 1
    masks = codec.usable_masks(frags, obj_len)
    assert bin(masks[1]).count("1") == k + m - 5
    with pytest.raises(X.ECInsufficientFragments):
        codec.decode(frags, obj_len, masks, out)


def test_verify_report_and_argument_checks(oracle, gpu):
    import ctypes

    import torch
    from pyeclib_amd import _native, batch
    from pyeclib_amd import exceptions as X
    k, m, obj_len, n_obj = 4, 2, 4104, 4
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    _, frags, bs = encode_stripes(codec, gpu, obj_len, n_obj)
    frags[1, 3, HDR + 1025] ^= 1
    frags[1, 0, HDR] ^= 1
    frags[2, 5, HDR + 7] ^= 1   # a bad checksum next to ...
    frags[2, 1, 12] ^= 1        # ... a bad header: the header is reported
    frags[3, 2, 53] = 1         # chksum_mismatch flag, metadata checksum recomputed
    h = bytearray(frags[3, 2, :HDR].cpu().numpy().tobytes())
    frags[3, 2, :HDR] = torch.from_numpy(np.frombuffer(bytes(remeta(oracle, h)), dtype=np.uint8).copy()).to(gpu)
    assert codec.verify_report(frags, obj_len) == [
        {"status": 0},
        {"status": -205, "reason": "Bad checksum", "bad_fragments": [0, 3]},
        {"status": -207, "reason": "Bad header", "bad_fragments": [1]},
        {"status": -205, "reason": "Bad checksum", "bad_fragments": [2]}]
    want = [[0, 0], [0, 0b1001], [1 << 1, 1 << 5], [0, 1 << 2]]
    assert expected(oracle, frags.cpu().numpy(), "amd_rs_vand", bs, obj_len) == want
    # n_obj = 0: nothing to do
    assert tuple(codec.verify(frags, obj_len, present_masks=[]).shape) == (0, 2)
    assert _native.lib.ecamd_verify_batch(codec.handle.desc, frags.data_ptr(), frags.stride(1),
                                          frags.stride(0), obj_len, 0, None, None, None) == 0
    # guards: a fragment stride below 80 + round16(bs), more objects than
    # the buffer holds, null pointers
    small = torch.zeros((n_obj, k + m, HDR + r16(bs) - 16), dtype=torch.uint8, device=gpu)
    with pytest.raises(X.ECInvalidParameter):
        codec.verify(small, obj_len)
    with pytest.raises(X.ECInvalidParameter):
        codec.verify(frags, obj_len, present_masks=[1] * (n_obj + 1))
    res = torch.zeros((n_obj, 2), dtype=torch.int32, device=gpu)
    masks = (ctypes.c_uint32 * n_obj)(*([63] * n_obj))
    for d_frags, d_res in ((None, res.data_ptr()), (frags.data_ptr(), None)):
        assert _native.lib.ecamd_verify_batch(
            codec.handle.desc, d_frags, frags.stride(1), frags.stride(0), obj_len, n_obj, masks,
            d_res, None) == -_native.EINVALIDPARAMS
