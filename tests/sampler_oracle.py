"""Which rows a ReservoirSampler keeps — a Python restatement of the selection, independent of the library's C++.

Built from two sources only: the recipe of the draws in include/frostdb_amd.h (splitmix64 seeded with the caller's seed; a unit draw is
((x >> 11) + 0.5) * 2^-53, a slot draw (x * size) >> 64, the skip is 1 where 1 - w rounds to 0) and the control flow of the reference's
ReservoirSampler (fill, then sample: the `s.i == 0` sentinel, the pending index carried into the next record, one slot draw and one
update of w per replacement). ``sample(seed, size, lens)`` returns, per slot, the row it ends with, numbered across the records in push
order. math.log / math.exp are the C library's, like the library's own.
"""
import math

_M = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.x = seed & _M

    def u64(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & _M
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
        return z ^ (z >> 31)

    def unit(self):  # ≙ rand.Float64(), never 0
        return ((self.u64() >> 11) + 0.5) * 2.0 ** -53

    def below(self, n):  # ≙ rand.Intn(n)
        return (self.u64() * n) >> 64


def sample(seed, size, lens):
    rng = SplitMix64(seed)
    reservoir = []
    n = 0      # s.n: rows seen
    i = 0.0    # s.i
    w = math.exp(math.log(rng.unit()) / size) if size > 0 else 0.0  # NewReservoirSampler
    base = 0   # rows of the records before this one

    def next_w(w):
        return w * math.exp(math.log(rng.unit()) / size)

    for rows in lens:
        if rows == 0:  # a zero-row push is a no-op
            continue
        lo = 0
        if n < size:  # fill(): whole record, or the part that still fits
            t = min(rows, size - n)
            reservoir.extend(base + k for k in range(t))
            n += t
            lo = t
        if lo < rows and size > 0:  # sample() over the slice [lo, rows): its row r is row base + lo + r
            first = base + lo
            nn = n + (rows - lo)
            if i == 0:
                i = float(n) - 1
            elif i < nn:
                reservoir[rng.below(size)] = first + int(i) - n
                w = next_w(w)
            while i < nn:
                d = math.log(1 - w) if w < 1 else -math.inf
                i += math.floor(math.log(rng.unit()) / d) + 1
                if i < nn:
                    reservoir[rng.below(size)] = first + int(i) - n
                    w = next_w(w)
            n = nn
        base += rows
    return reservoir
