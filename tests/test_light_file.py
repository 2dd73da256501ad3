"""Light accumulator checkpoints (rt4_light_save / rt4_light_info / rt4_light_load, include/rt4.h) on the CPU: byte-exact
round trips, padded strides, the header's layout and the error paths, in the manner of test_accum.py."""
import ctypes
import os

import numpy as np
import pytest

HEADER = 44  # "RT4LIT1\0", int32 version, w, h, int64 frames_issued, uint32 seed, key, flags, 0


def random_acc(rt4, h, w, seed=5):
    rng = np.random.default_rng(seed)
    acc = np.frombuffer(rng.bytes(h * w * 32), rt4.LIGHT_DTYPE).reshape(h, w).copy()  # any bits: NaNs, negative n
    return acc


def test_round_trip_is_byte_exact(rt4, tmp_path):
    acc = random_acc(rt4, 17, 33)
    path = str(tmp_path / "l.rt4l")
    rt4.light_save(path, acc, frames_issued=2 ** 33 + 5, seed=0xDEADBEEF, key=0x12345678, flags=rt4.LIGHT_POOLED)
    assert not os.path.exists(path + ".tmp")
    assert os.path.getsize(path) == HEADER + acc.nbytes  # header + rows without padding
    want = {"w": 33, "h": 17, "frames_issued": 2 ** 33 + 5, "seed": 0xDEADBEEF, "key": 0x12345678, "flags": 1}
    assert rt4.light_info(path) == want
    back, info = rt4.light_load(path)
    assert info == want and back.dtype == acc.dtype and back.shape == acc.shape and back.tobytes() == acc.tobytes()


def test_padded_stride_and_header_layout(rt4, tmp_path):
    h, w, stride = 5, 7, 10
    buf = random_acc(rt4, h, stride)
    path = str(tmp_path / "s.rt4l")
    rt4.light_save(path, buf, frames_issued=3, seed=9, key=4, w=w)
    raw = open(path, "rb").read()
    assert raw[:8] == b"RT4LIT1\0"
    version, fw, fh, issued, seed, key, flags, zero = np.frombuffer(raw[8:HEADER], dtype="<i4,<i4,<i4,<i8,<u4,<u4,<u4,<u4")[0]
    assert (version, fw, fh, issued, seed, key, flags, zero) == (1, w, h, 3, 9, 4, 0, 0)
    pixels = np.frombuffer(raw[HEADER:], rt4.LIGHT_DTYPE).reshape(h, w)
    assert pixels.tobytes() == np.ascontiguousarray(buf[:, :w]).tobytes()  # the padding columns are not stored
    out = random_acc(rt4, h, stride, seed=6)
    before = out.copy()
    _, info = rt4.light_load(path, out, w=w)
    assert np.ascontiguousarray(out[:, :w]).tobytes() == pixels.tobytes()
    assert np.ascontiguousarray(out[:, w:]).tobytes() == np.ascontiguousarray(before[:, w:]).tobytes()
    assert (info["frames_issued"], info["seed"], info["key"], info["flags"]) == (3, 9, 4, 0)


def test_errors(rt4, tmp_path):
    lib = rt4.lib
    err = ctypes.create_string_buffer(256)
    acc = random_acc(rt4, 4, 4)
    good = str(tmp_path / "g.rt4l")
    rt4.light_save(good, acc, 2, 1)
    raw = open(good, "rb").read()

    def load_into(path, out, w, h):
        return lib.rt4_light_load(os.fsencode(path), ctypes.c_void_p(out.ctypes.data), w, h, out.shape[1], None, None, None,
                                  None, err, len(err))

    # another w or h on load: RT4_ERR_ARG, buffer untouched
    for w, h in ((5, 4), (4, 5), (3, 4)):
        out = random_acc(rt4, h, w, seed=8)
        before = out.tobytes()
        assert load_into(good, out, w, h) == -1 and b"4x4" in err.value and out.tobytes() == before
    # not a light checkpoint (a colour checkpoint too), truncated, too long, another version, a bad header: RT4_ERR_PARSE
    cases = {"magic": b"RT4ACC1\0" + raw[8:], "short": raw[:-16], "header": raw[:20], "long": raw + bytes(32),
             "version": raw[:8] + (2).to_bytes(4, "little") + raw[12:], "width": raw[:12] + (5).to_bytes(4, "little") + raw[16:],
             "zero": raw[:40] + (1).to_bytes(4, "little") + raw[44:]}
    match = {"magic": "not an rt4 light checkpoint", "short": "truncated", "header": "not an rt4 light checkpoint",
             "long": "bytes", "version": "version 2", "width": "bytes", "zero": "bad light checkpoint header"}
    for name, data in cases.items():
        p = tmp_path / (name + ".rt4l")
        p.write_bytes(data)
        with pytest.raises(rt4.RT4Error, match=match[name]) as ei:
            rt4.light_info(str(p))
        assert ei.value.status == -3, name  # RT4_ERR_PARSE
        out = random_acc(rt4, 4, 4, seed=8)
        before = out.tobytes()
        assert load_into(str(p), out, 4, 4) == -3 and out.tobytes() == before, name
    with pytest.raises(rt4.RT4Error, match="cannot open"):
        rt4.light_info(str(tmp_path / "missing.rt4l"))
    # bad arguments on save: a stride below w, negative frames_issued, a NULL accumulator
    p = ctypes.c_void_p(acc.ctypes.data)
    assert lib.rt4_light_save(os.fsencode(good), p, 4, 4, 3, 0, 0, 0, 0, err, len(err)) == -1
    assert lib.rt4_light_save(os.fsencode(good), p, 4, 4, 4, -1, 0, 0, 0, err, len(err)) == -1
    assert lib.rt4_light_save(os.fsencode(good), None, 4, 4, 4, 0, 0, 0, 0, err, len(err)) == -1
    assert open(good, "rb").read() == raw


def test_failed_save_keeps_the_previous_checkpoint(rt4, tmp_path):
    path = str(tmp_path / "ck.rt4l")
    rt4.light_save(path, random_acc(rt4, 6, 9), 4, 77)
    before = open(path, "rb").read()
    os.mkdir(path + ".tmp")
    with pytest.raises(rt4.RT4Error, match="cannot open"):
        rt4.light_save(path, random_acc(rt4, 6, 9, seed=2), 5, 77)
    assert open(path, "rb").read() == before
    os.rmdir(path + ".tmp")
    rt4.light_save(path, random_acc(rt4, 6, 9, seed=2), 5, 77)
    assert rt4.light_info(path)["frames_issued"] == 5 and not os.path.exists(path + ".tmp")
