"""Reference of the beat detection (include/gdkvm.h, gdkvm_lv_beats) in plain Python integers: candidates with scipy's plateau rule, the GREEDY
form of the distance rule (the kernel iterates the fixed-point form), the prominence walks over all frames, the beats and their EF.  Floats
appear only where the definition has them, one IEEE operation at a time (Python floats are fp64 and never fused)."""


def end_systoles(a, distance, permille):
    """The end-systoles of the valid curve `a` (a list of ints), ascending."""
    n = len(a)
    cand = []
    p = 1
    while p < n - 1:
        if a[p - 1] > a[p]:
            r = p
            while r + 1 < n and a[r + 1] == a[p]:
                r += 1
            if r + 1 < n and a[r + 1] > a[p]:
                cand.append((p + r) // 2)
            p = r + 1
        else:
            p += 1
    kept, is_kept = [], [False] * n
    for c in sorted(cand, key=lambda c: (a[c], c)):          # priority: smaller area first, then the lower frame
        if not any(is_kept[max(0, c - distance + 1):c + distance]):      # no kept candidate q with |c - q| < distance
            kept.append(c)
            is_kept[c] = True
    rng = max(a) - min(a) if n else 0
    out = []
    for c in sorted(kept):
        lmax = rmax = a[c]
        j = c - 1
        while j >= 0 and a[j] >= a[c]:
            lmax = max(lmax, a[j])
            j -= 1
        j = c + 1
        while j < n and a[j] >= a[c]:
            rmax = max(rmax, a[j])
            j += 1
        if (min(lmax, rmax) - a[c]) * 1000 >= permille * rng:
            out.append(c)
    return out


def lv_beats_ref(area, vol, length=None, max_beats=16, distance=20, permille=500, min_pixels=1):
    """area, vol: [B][T]; length: [B] or None.  Returns (beats [B][max_beats][2], beat_val [B][max_beats][3], info [B][4], summ [B][4])."""
    beats, beat_val, info, summ = [], [], [], []
    for b in range(len(area)):
        T = len(area[b])
        n = T if length is None else min(max(int(length[b]), 0), T)
        a = [int(v) for v in area[b][:n]]
        v = [float(x) for x in vol[b][:n]]
        es = end_systoles(a, distance, permille)
        rows, prev = [], -1
        for j, e in enumerate(es):
            seg = a[prev + 1:e]
            ed = prev + 1 + seg.index(max(seg))               # the lowest frame of the largest area
            if not (j == 0 and ed == 0):
                edv, esv = v[ed], v[e]
                rows.append((ed, e, edv, esv, 0.0 if edv == 0.0 else (edv - esv) / edv))
            prev = e
        m = len(es)
        span = es[-1] - es[0] if m else 0
        bt = [[r[0], r[1]] for r in rows[:max_beats]]
        bv = [[r[2], r[3], r[4]] for r in rows[:max_beats]]
        beats.append(bt + [[-1, -1]] * (max_beats - len(bt)))
        beat_val.append(bv + [[0.0, 0.0, 0.0]] * (max_beats - len(bv)))
        info.append([len(rows), m, sum(1 for x in a if x < min_pixels), span])
        if rows:
            s = 0.0
            for r in rows:
                s = s + r[4]
            summ.append([s / float(len(rows)), min(r[4] for r in rows), max(r[4] for r in rows), 0.0 if m < 2 else float(span) / float(m - 1)])
        else:
            summ.append([0.0, 0.0, 0.0, 0.0])
    return beats, beat_val, info, summ
