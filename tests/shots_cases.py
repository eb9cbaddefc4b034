"""Synthetic sequences for the scene-cut tests (CPU and GPU): 24 x 40 uint8 frames, each shot the pattern
128 + 100 sin(fx x + phi) cos(fy y + phi) panned `pan` pixels per frame under sigma = 2 noise, with fx, fy and phi drawn per shot from a
seeded generator.  Nothing here depends on the code under test."""
import numpy as np

H, W = 24, 40
SEEDS = (3, 17, 41)                        # the fixed seed sets of the known-answer tests
LENGTHS = (5, 3, 9, 6)                     # shot lengths: cuts at 5, 8 and 17
CUTS = [5, 8, 17]


def _pattern(rs):
    return rs.uniform(0.15, 0.6), rs.uniform(0.15, 0.6), rs.uniform(0.0, 2 * np.pi)


def _frame(par, shift, rs, size=(H, W)):
    fx, fy, phi = par
    yy, xx = np.mgrid[0:size[0], 0:size[1]].astype(np.float64)
    return 128.0 + 100.0 * np.sin(fx * (xx + shift) + phi) * np.cos(fy * yy + phi) + rs.normal(0.0, 2.0, size)


def _u8(frames):
    return np.clip(np.rint(np.stack(frames, 0)), 0, 255).astype(np.uint8)[:, None]


def shots_sequence(seed, lengths=LENGTHS, pan=1, size=(H, W)):
    """(sum(lengths), 1, *size) uint8: one shot per entry of `lengths`, panned `pan` pixels per frame."""
    rs = np.random.RandomState(seed)
    frames = []
    for n in lengths:
        par = _pattern(rs)
        frames += [_frame(par, pan * t, rs, size) for t in range(n)]
    return _u8(frames)


def crossfade_sequence(seed, head=4, fade=12, tail=4):
    """Two shots joined by a `fade`-frame linear cross-fade (both keep panning through it)."""
    rs = np.random.RandomState(seed)
    a, b = _pattern(rs), _pattern(rs)
    n = head + fade + tail
    frames = []
    for t in range(n):
        w = min(max((t - head + 1) / (fade + 1), 0.0), 1.0)
        frames.append((1 - w) * _frame(a, t, rs) + w * _frame(b, t, rs))
    return _u8(frames)


def ten_bit(frames_u8):
    """The 10-bit copy 4k + 1 of 8-bit frames, uint16."""
    return frames_u8.astype(np.uint16) * 4 + 1
