"""Numpy restatement of the observation tensors (include/doomgpu.h: dg_obs_desc), written from the contract's text.  Per element:
  1. v: np_reduce.reduce's byte (RGB, or GRAY), or np_plane_reduce.reduce's distance as the signed int16 it is;
  2. v = min(max(v, lo), hi);
  3. U8: the element is v.  Otherwise o = float32(float32(v) * scale) + bias in np.float32 arithmetic (numpy rounds after each operation
     and keeps subnormals); F32 stores o, F16 o.astype(np.float16), BF16 round-to-nearest-even by integer arithmetic on the float32 bits;
  4. the element goes to base + n*s0 + c*s1 + oy*s2 + ox*s3 (in elements).
Everything is returned and compared as unsigned BIT PATTERNS (uint8 / uint16 / uint32), so that signed zeros and infinities are pinned."""
import numpy as np

import np_plane_reduce as npp
import np_reduce as npr

RGB, GRAY, DISTANCE = 0, 1, 2
U8, F16, BF16, F32 = 0, 1, 2, 3
DTYPES = (U8, F16, BF16, F32)
BITS = {U8: np.uint8, F16: np.uint16, BF16: np.uint16, F32: np.uint32}          # the unsigned type of an element's bit pattern
DTYPE_NAMES = {U8: "uint8", F16: "float16", BF16: "bfloat16", F32: "float32"}
# (source, rule): the four kinds of observation
KINDS = ((RGB, 0), (GRAY, 0), (DISTANCE, npp.POINT), (DISTANCE, npp.NEAREST))
FULL = (-32768, 32767)


def channels(source):
    return 3 if source == RGB else 1


def values(source, rule, fx, fy, src):
    """Step 1: (n, C, oH, oW) int64 from frames (n, H, W, 3) uint8 or distance planes (n, H, W) int16."""
    if source == DISTANCE:
        return npp.reduce(rule, fx, fy, distance=src)["distance"].astype(np.int64)[:, None]
    if source == GRAY:
        return npr.reduce(src, fx, fy, npr.GRAY8).astype(np.int64)[:, None]
    return npr.reduce(src, fx, fy, npr.RGB24).astype(np.int64).transpose(0, 3, 1, 2)


def bf16_bits(bits32):
    """float32 bit patterns (uint32) -> bfloat16 bit patterns (uint16), round to nearest even; a NaN becomes the quiet 0x7FC0."""
    u = np.asarray(bits32, dtype=np.uint32).astype(np.uint64)
    out = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    out = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC0, out)
    return out.astype(np.uint16)


def convert(v, dtype, lo, hi, scale, bias):
    """Steps 2 and 3 on integer values of any shape: the elements' bit patterns."""
    v = np.clip(np.asarray(v, dtype=np.int64), lo, hi)
    if dtype == U8:
        assert scale == 1 and bias == 0 and 0 <= lo and hi <= 255
        return v.astype(np.uint8)
    with np.errstate(over="ignore", under="ignore"):
        o = v.astype(np.float32) * np.float32(scale)
        o = o + np.float32(bias)
        assert o.dtype == np.float32
        if dtype == F32:
            return o.view(np.uint32)
        if dtype == F16:
            return o.astype(np.float16).view(np.uint16)
    return bf16_bits(o.view(np.uint32))


def observe(src, source, rule, fx, fy, dtype, lo, hi, scale, bias):
    return convert(values(source, rule, fx, fy, src), dtype, lo, hi, scale, bias)


# ---- the destination layouts both tiers run ------------------------------------------------------------------------------------------
LAYOUTS = ("nchw", "nhwc", "slice")


def layout(name, n, C, oH, oW):
    """(elements of the whole buffer, element offset of (0,0,0,0), strides in elements).  nchw: contiguous; nhwc: channels-last; slice:
    channels 1..1+C of an (n, C+2, oH+1, oW+3) buffer whose frame stride is one observation larger than it needs."""
    if name == "nchw":
        return n * C * oH * oW, 0, (C * oH * oW, oH * oW, oW, 1)
    if name == "nhwc":
        return n * C * oH * oW, 0, (oH * oW * C, 1, oW * C, C)
    assert name == "slice"
    plane = (oH + 1) * (oW + 3)
    frame = (C + 2) * plane + C * oH * oW
    return n * frame, plane, (frame, plane, oW + 3, 1)


def addresses(shape, base, strides):
    n, C, oH, oW = shape
    i = np.ix_(np.arange(n), np.arange(C), np.arange(oH), np.arange(oW))
    return base + i[0] * strides[0] + i[1] * strides[1] + i[2] * strides[2] + i[3] * strides[3]


def sentinel(total, dtype):
    """A buffer of `total` elements of the dtype's bit-pattern type, every byte 0xA5."""
    return np.full(total * np.dtype(BITS[dtype]).itemsize, 0xA5, dtype=np.uint8).view(BITS[dtype])


def placed(bits, name):
    """The model's (n, C, oH, oW) bit patterns in layout `name`: (the whole expected buffer, sentinel elements around, base, strides)."""
    dtype_bits = bits.dtype
    total, base, strides = layout(name, *bits.shape)
    buf = np.full(total * dtype_bits.itemsize, 0xA5, dtype=np.uint8).view(dtype_bits)
    at = addresses(bits.shape, base, strides)
    assert np.unique(at).size == at.size and at.max(initial=0) < max(total, 1)
    buf[at.reshape(-1)] = bits.reshape(-1)
    return buf, base, strides


# ---- the maps both tiers run: (scale, bias, lo, hi, which sources it is for) --------------------------------------------------------------
F = np.float32
MAPS = {
    "identity": (F(1), F(0), *FULL),
    "unit": (F(1) / F(255), F(0), *FULL),
    "signed": (F(2) / F(255), F(-1), *FULL),
    "negate": (F(-1), F(0), *FULL),                      # signed zero: 0 * -1 + 0 = +0
    "f32_subnormal": (F(2.0 ** -140), F(0), *FULL),
    "f16_subnormal": (F(2.0 ** -20), F(0), *FULL),
    "f16_infinity": (F(1000), F(0), *FULL),
    "f32_infinity": (F(1e36), F(0), *FULL),              # on distances: 32767e36 is beyond float32
    "far": (F(1) / F(2048), F(0), 0, 2048),              # depth with a far clamp
    "lo_eq_hi": (F(3), F(0.5), 77, 77),
}
U8_MAPS = {"u8_full": (F(1), F(0), 0, 255), "u8_window": (F(1), F(0), 10, 200), "u8_lo_eq_hi": (F(1), F(0), 77, 77)}


def maps_for(dtype):
    return U8_MAPS if dtype == U8 else MAPS


def sources(source, n, W, H, fx, fy):
    """n frames of the kind's source, cycling through the tiers' contents: np_reduce.CONTENTS for colour, np_plane_reduce's for distance."""
    if source == DISTANCE:
        each = [npp.distance_content(k, 1, W, H, fx, fy, seed=i) for i, k in enumerate(npp.CONTENTS)]
    else:
        each = [npr.content(k, 1, W, H, seed=i) for i, k in enumerate(npr.CONTENTS)]
    return np.concatenate([each[i % len(each)] for i in range(n)])


def sweep_frame():
    """One 256x256 distance frame that holds every int16 once."""
    return (np.arange(65536, dtype=np.int64) - 32768).astype(np.int16).reshape(1, 256, 256)


def structured_f32_patterns():
    """More than 10^6 float32 bit patterns: every exponent x mantissa patterns at the edges of both narrowings (the bits around the 13
    and the 16 that are rounded away, all-ones runs, ties and their neighbours) x both signs."""
    m = set()
    for cut in (13, 16, 23):                                          # bits rounded away: float16, bfloat16, and (float16 subnormals) all
        for keep in range(0, 64):                                     # the low kept bits ...
            for low in (0, 1, (1 << (cut - 1)) - 1, 1 << (cut - 1), (1 << (cut - 1)) + 1, (1 << cut) - 1):     # ... x below / at / above a tie
                m.add(((keep << cut) | low) & 0x7FFFFF)
                m.add((0x7FFFFF ^ ((keep << cut) | low)) & 0x7FFFFF)
    for k in range(24):
        m.update(((1 << k) & 0x7FFFFF, ((1 << k) - 1) & 0x7FFFFF, (0x7FFFFF >> k), (0x7FFFFF >> k) ^ 1, (0x7FFFFF << k) & 0x7FFFFF))
    m.update(int(x) for x in np.random.default_rng(1993).integers(0, 1 << 23, size=1200))
    mant = np.array(sorted(m), dtype=np.uint32)
    exp = np.arange(256, dtype=np.uint32)
    pos = ((exp[:, None] << 23) | mant[None, :]).reshape(-1)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])
