"""The adaptive gather's rule (include/ptmi_plugin.h Part 19) restated in numpy from the header comment of
csrc/adaptive_gather_rule.h: every operation is one float32 operation in the order the text gives, whole lists at a time."""
import numpy as np

F = np.float32
ACTIVE, BY_THRESHOLD, BY_MAX_SAMPLES, NON_FINITE = 0, 1, 2, 3
MAX_COUNT = 1 << 24


def luminance(e):
    return (e[..., 0] * F(0.299) + e[..., 1] * F(0.587)) + e[..., 2] * F(0.114)


def variance_of_mean(l, m2, n):
    """v of step 2; n: one count or an array of counts"""
    S = np.asarray(n).astype(F)
    with np.errstate(all="ignore"):
        return np.fmax((m2 - (S * l) * l) / (S - F(1.0)), F(0.0)) / S


def reasons(acc, n, add_samples, max_samples, threshold, dark_floor):
    """step 2 for every row of acc ((k, 4) float32 of n samples each): ACTIVE or why the entry stops"""
    acc = np.ascontiguousarray(acc, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        l = luminance(acc[:, :3])
        v = variance_of_mean(l, acc[:, 3], n)
        d = np.fmax(l, F(dark_floor))
        noisy = v > (F(threshold) * F(threshold)) * (d * d)
    out = np.where(noisy, BY_MAX_SAMPLES if n + add_samples > max_samples else ACTIVE, BY_THRESHOLD)
    return np.where(np.isfinite(acc).all(axis=1), out, NON_FINITE)


def select(acc, recv, n, add_samples, max_samples, threshold, dark_floor, active=None):
    """(indices that go on, their receivers, stopped (3,): by threshold, by max_samples, non-finite)"""
    acc = np.ascontiguousarray(acc, F).reshape(-1, 4)
    recv = np.ascontiguousarray(recv, F).reshape(-1, 8)
    idx = np.arange(len(acc), dtype=np.uint32) if active is None else np.asarray(active, np.uint32).reshape(-1)
    r = reasons(acc[idx], n, add_samples, max_samples, threshold, dark_floor)
    keep = idx[r == ACTIVE]
    return keep, recv[keep], np.array([(r == k).sum() for k in (BY_THRESHOLD, BY_MAX_SAMPLES, NON_FINITE)], np.uint64)


def fold(acc, n, fresh, m, active=None, counts=None):
    """step 3: fresh (m samples) into the rows of acc (n samples; 0 writes) that active names; returns new arrays"""
    acc = np.array(acc, F).reshape(-1, 4)
    fresh = np.ascontiguousarray(fresh, F).reshape(-1, 4)
    idx = np.arange(len(acc)) if active is None else np.asarray(active, np.int64).reshape(-1)
    if n == 0:
        acc.view(np.uint32)[idx] = fresh.view(np.uint32)
    else:
        with np.errstate(all="ignore"):
            acc[idx, :3] = (acc[idx, :3] * F(n) + fresh[:, :3] * F(m)) / F(n + m)
            acc[idx, 3] = acc[idx, 3] + fresh[:, 3]
    if counts is None:
        return acc
    counts = np.array(counts, np.uint32)
    counts[idx] = n + m
    return acc, counts


def equalise(irr, counts, samples_eq):
    """step 5"""
    irr = np.ascontiguousarray(irr, F).reshape(-1, 4)
    counts = np.asarray(counts, np.uint32).reshape(-1)
    out = irr.copy()
    ok = np.isfinite(irr).all(axis=1) & (counts >= 2) & (counts <= MAX_COUNT)
    with np.errstate(all="ignore"):
        l = luminance(irr[:, :3])
        v = variance_of_mean(l, irr[:, 3], np.where(ok, counts, 2))
        S = F(samples_eq)
        m2 = (S * l) * l + (v * S) * (S - F(1.0))
    out.view(np.uint32)[ok, 3] = m2.astype(F).view(np.uint32)[ok]
    return out


def adaptive(gather, count, first_sample, min_samples, add_samples, max_samples, threshold, dark_floor, recv=None):
    """The whole loop from `gather(first_sample, samples) -> (count, 4) rows of EVERY entry`: what PTGatherIrradianceAdaptive returns
    when a gather of an entry does not depend on its neighbours in the list.  Returns (irradiance, counts, stats)."""
    recv = np.zeros((count, 8), F) if recv is None else recv
    acc = fold(np.zeros((count, 4), F), 0, gather(first_sample & 0xFFFFFFFF, min_samples), min_samples)
    counts = np.full(count, min_samples, np.uint32)
    n, first = min_samples, first_sample + min_samples
    stats = dict(rounds=1, samples=count * min_samples, stoppedThreshold=0, stoppedMaxSamples=0, stoppedNonFinite=0)
    active, _, stopped = select(acc, recv, n, add_samples, max_samples, threshold, dark_floor)
    while True:
        for k, name in enumerate(("stoppedThreshold", "stoppedMaxSamples", "stoppedNonFinite")):
            stats[name] += int(stopped[k])
        if not len(active):
            break
        fresh = gather(first & 0xFFFFFFFF, add_samples)[active]
        acc, counts = fold(acc, n, fresh, add_samples, active, counts)
        n, first = n + add_samples, first + add_samples
        stats["rounds"] += 1
        stats["samples"] += len(active) * add_samples
        active, _, stopped = select(acc, recv, n, add_samples, max_samples, threshold, dark_floor, active)
    stats["maxCount"] = n
    return acc, counts, stats
