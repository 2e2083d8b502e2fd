"""Differentiable discriminator augmentation: the policy string and a pure-Python mirror of ``him_diffaug_draw``.

The device draws the parameter table itself (``ops.diffaug_draw``); ``draw`` below restates the construction written
down in include/him.h in integers and returns the same (B, 8) rows, bit for bit.  It needs neither torch nor the library.
"""
import math
import struct

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
POLICY_BITS = {'color': COLOR, 'translation': TRANSLATION, 'cutout': CUTOUT}
_M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def parse_policy(text):
    """'' -> 0 (off); a comma list out of color, translation, cutout -> the policy bits.  Anything else raises."""
    if text is None:
        return 0
    if not isinstance(text, str):
        raise ValueError('--diffaug takes a string, got %r' % (text,))
    bits = 0
    if text.strip() == '':
        return 0
    for name in text.split(','):
        name = name.strip()
        if name not in POLICY_BITS:
            raise ValueError("--diffaug: unknown augmentation %r (a comma list out of color, translation, cutout)" % name)
        bits |= POLICY_BITS[name]
    return bits


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _f32_bits(v):
    """``v`` (exact in double) rounded to fp32 once, as the int32 holding its bits."""
    return struct.unpack('<i', struct.pack('<f', v))[0]


def _randint(z, lo, hi):
    return lo + (((z >> 32) * (hi - lo + 1)) >> 32)


def sizes(H, W, policy, ratio_translation=0.125, ratio_cutout=0.5):
    """-> (sy, sx, ch, cw): the largest shifts and the cutout size (0, 0 without the cutout bit)."""
    sy, sx = int(math.floor(H * ratio_translation + 0.5)), int(math.floor(W * ratio_translation + 0.5))
    if policy & CUTOUT:
        return sy, sx, int(math.floor(H * ratio_cutout + 0.5)), int(math.floor(W * ratio_cutout + 0.5))
    return sy, sx, 0, 0


def draw(B, H, W, seed, step, sample0, policy, ratio_translation=0.125, ratio_cutout=0.5):
    """-> (rows, ch, cw): rows is a list of B lists of 8 ints, [bits(b), bits(a), bits(k), ty, tx, cut_y0, cut_x0, policy]."""
    sy, sx, ch, cw = sizes(H, W, policy, ratio_translation, ratio_cutout)
    rows = []
    for b in range(B):
        key = _mix((seed + _G) & _M64)
        key = _mix((key + step + _G) & _M64)
        key = _mix((key + sample0 + b + _G) & _M64)
        z = [_mix((key + (i + 1) * _G) & _M64) for i in range(7)]
        u = [(zi >> 40) * 2.0 ** -24 for zi in z[:3]]
        fb, fa, fk, ty, tx, cy, cx = 0.0, 1.0, 1.0, 0, 0, 0, 0
        if policy & COLOR:
            fb, fa, fk = u[0] - 0.5, 2.0 * u[1], u[2] + 0.5
        if policy & TRANSLATION:
            ty, tx = _randint(z[3], -sy, sy), _randint(z[4], -sx, sx)
        if policy & CUTOUT:
            cy = _randint(z[5], 0, H - (ch & 1)) - ch // 2
            cx = _randint(z[6], 0, W - (cw & 1)) - cw // 2
        rows.append([_f32_bits(fb), _f32_bits(fa), _f32_bits(fk), ty, tx, cy, cx, policy & 7])
    return rows, ch, cw
