"""The definition of gdkvm_temporal_vote (include/gdkvm.h) restated in numpy: one-hot window sums for whole clips, and a plain loop over one
pixel's labels against which the tests check those sums.  Nothing here knows about packed bytes, keys or lanes.  Also the input recipe of the
GPU tests (a blob per clip that drifts over the frames, 15 % of the pixels re-drawn over the classes, 1 % set to 255) and the hand-built
pixels of the CPU test, planted into the first pixels of a clip."""
import numpy as np


def vote_pixel(labels, t, ncls, radius):
    """out of ONE pixel at frame t; `labels` are its bytes over the T frames of its clip."""
    own = int(labels[t])
    if own >= ncls:
        return own                                                 # rule 3: pass-through
    votes = [0] * ncls
    for u in range(max(0, t - radius), min(len(labels) - 1, t + radius) + 1):     # rule 1: truncated, not padded
        if int(labels[u]) < ncls:                                  # rule 2
            votes[int(labels[u])] += 1
    most = max(votes)
    if votes[own] == most:                                         # rule 4: the own label wins a tie it is part of ...
        return own
    return votes.index(most)                                       # ... else the smallest class


def temporal_vote_ref(mask, ncls, radius, target=None):
    """mask [clips, T, H, W] uint8 -> (out uint8, info int32 [clips, T, 4], counts int32 [clips, T, ncls, 3] or None)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 4
    B, T, H, W = mask.shape
    onehot = (mask[..., None] == np.arange(ncls, dtype=np.uint8)).astype(np.int8)            # [B, T, H, W, C]; a window has at most 15 frames
    out = mask.copy()
    for t in range(T):
        votes = onehot[:, max(0, t - radius):min(T - 1, t + radius) + 1].sum(1, dtype=np.int8)             # [B, H, W, C]
        own = mask[:, t]
        valid = own < ncls
        most = votes.max(-1)
        own_votes = np.take_along_axis(votes, np.minimum(own, ncls - 1)[..., None].astype(np.int64), -1)[..., 0]
        smallest = votes.argmax(-1).astype(np.uint8)               # argmax returns the first, i.e. the smallest, index of the maximum
        out[:, t] = np.where(valid, np.where(own_votes == most, own, smallest), own)
    info = np.zeros((B, T, 4), np.int32)
    info[..., 0] = (out != mask).sum((2, 3))
    info[:, 1:, 1] = (mask[:, 1:] != mask[:, :-1]).sum((2, 3))
    info[:, 1:, 2] = (out[:, 1:] != out[:, :-1]).sum((2, 3))
    counts = None
    if target is not None:
        target = np.asarray(target)
        assert target.shape == mask.shape and target.dtype == np.uint8
        counts = np.zeros((B, T, ncls, 3), np.int32)
        for c in range(ncls):
            o, g = out == c, target == c
            counts[:, :, c, 0] = (o & g).sum((2, 3))
            counts[:, :, c, 1] = o.sum((2, 3))
            counts[:, :, c, 2] = g.sum((2, 3))
    return out, info, counts


def tie_kinds(mask, ncls, radius):
    """(ties the own label won, ties it was no part of, bytes >= ncls passed through) over every pixel and frame: what a test asserts to be
    non-zero before it trusts a comparison."""
    mask = np.asarray(mask)
    T = mask.shape[1]
    onehot = (mask[..., None] == np.arange(ncls, dtype=np.uint8)).astype(np.int8)
    own_ties = other_ties = 0
    for t in range(T):
        votes = onehot[:, max(0, t - radius):min(T - 1, t + radius) + 1].sum(1, dtype=np.int8)
        own = mask[:, t]
        valid = own < ncls
        most = votes.max(-1)
        tied = (votes == most[..., None]).sum(-1) > 1
        own_in = np.take_along_axis(votes, np.minimum(own, ncls - 1)[..., None].astype(np.int64), -1)[..., 0] == most
        own_ties += int((valid & tied & own_in).sum())
        other_ties += int((valid & tied & ~own_in).sum())
    return own_ties, other_ties, int((mask >= ncls).sum())


def drifting_clips(clips, T, H, W, ncls, seed):
    """The GPU tests' recipe: per clip an elliptic blob of one foreground class that drifts and breathes over the frames inside a ring of the
    next class (when there is one), 15 % of all pixels re-drawn uniformly over the classes, 1 % set to 255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((clips, T, H, W), np.uint8)
    for b in range(clips):
        fg = 1 + b % (ncls - 1)
        ring = 1 + (b + 1) % (ncls - 1)
        cy, cx = H / 2 + rng.uniform(-0.1, 0.1) * H, W / 2 + rng.uniform(-0.1, 0.1) * W
        dy, dx = rng.uniform(-0.03, 0.03) * H, rng.uniform(-0.03, 0.03) * W
        for t in range(T):
            s = 1.0 + 0.15 * np.sin(2 * np.pi * t / max(T, 2))
            d = ((yy - cy - dy * t) / (H / 3.2 * s + 0.5)) ** 2 + ((xx - cx - dx * t) / (W / 3.6 * s + 0.5)) ** 2
            m[b, t][d < 1.4] = ring
            m[b, t][d < 1.0] = fg
    noise = rng.random(m.shape) < 0.15
    m[noise] = rng.integers(0, ncls, int(noise.sum()), dtype=np.uint8)
    m[rng.random(m.shape) < 0.01] = 255
    return m


def plant_hand_pixels(mask, ncls, radius):
    """Writes hand-built label sequences like those of the CPU test into the first pixels (linear index 0..3 of a frame) of clip 0, where clip
    and frame are large enough to hold them.  Returns {name: (pixel, frame, the label `out` must have there)}.  In place."""
    B, T, H, W = mask.shape
    flat = mask.reshape(B, T, H * W)
    planted = {}
    n0 = min(radius, T - 1) + 1                                    # frames in the (truncated) window of frame 0
    if H * W >= 1 and n0 >= 2 and (n0 % 2 == 0 or ncls >= 3):
        # pixel 0: in the window of frame 0 the own label 1 and label 0 have as many votes (an odd window has one frame of 2 besides): 1 stays
        k = n0 // 2
        flat[0, :k, 0] = 1
        flat[0, k:2 * k, 0] = 0
        if n0 % 2:
            flat[0, 2 * k, 0] = 2
        planted["own tie"] = (0, 0, 1)
    if H * W >= 2 and radius >= 2 and T >= 2 * radius + 1 and ncls >= 3:
        # pixel 1: the full window of frame r holds r frames of 1, the own label 2 and r frames of 0: 0 and 1 tie without 2 -> 0
        flat[0, :radius, 1] = 1
        flat[0, radius, 1] = 2
        flat[0, radius + 1:2 * radius + 1, 1] = 0
        planted["other tie"] = (1, radius, 0)
    if H * W >= 3 and n0 >= 3:
        # pixel 2: the window of frame 0 is 1, 255 ... 255, 0: one vote each for 1 and 0, the own 1 stays -- unless a 255 voted for anything
        flat[0, 0, 2] = 1
        flat[0, 1:n0 - 1, 2] = 255
        flat[0, n0 - 1, 2] = 0
        planted["255 in the window"] = (2, 0, 1)
    elif H * W >= 3 and radius == 1 and T >= 3:
        # ... with r = 1 the window of frame 1: 0, 1, 255
        flat[0, 0, 2], flat[0, 1, 2], flat[0, 2, 2] = 0, 1, 255
        planted["255 in the window"] = (2, 1, 1)
    if H * W >= 4 and T >= 2:
        # pixel 3: 1 everywhere but a 255 at frame 1, which stays whatever its neighbours say
        flat[0, :, 3] = 1
        flat[0, 1, 3] = 255
        planted["255 at the centre"] = (3, 1, 255)
    return planted
