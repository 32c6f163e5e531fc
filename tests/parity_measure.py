"""What the per-entry float64 parity sweeps share: the bound, the seeded dyadic inputs, the error arithmetic and the table.
Plain numpy; neither torch nor the package, so a CPU test loads it in milliseconds.

An entry of a kernel's output is held to entry_bound(the fp32 composition's error at the same entry, s): s is the float64
restatement's sum of absolute summands behind the entry, u = 2^-24.  The form is derived, nothing in it was fitted.

Each sweep (tests/test_query_selection_parity_gpu.py, attn_parity.py, convnext_parity.py, tracker_parity.py, reid_parity.py,
loss_parity.py, vit_bwd_parity.py, convnext_bwd_parity.py, dec_bwd_parity.py, gemm_parity.py) keeps a `measure` of its own that decides what only it can: how a NaN or an infinity of the reference has to be
met, the key of its WORST, the format of its table line and which scale the project's tolerance multiplies.  It hands finite
arrays to errors() and takes the rest from here.  tests/test_parity_measure_cpu.py pins both halves.
"""
import os
import zlib

import numpy as np

U = 2.0 ** -24          # fp32 unit round-off
SUM_DEPTH = 16.0        # as tests/dynmask_cases.py: the bound's second term is SUM_DEPTH * U * s
COMP_MARGIN = 8.0       # and its first COMP_MARGIN x the fp32 composition's error of the same entry


def entry_bound(comp_err, mag):
    """The absolute form of max(COMP_MARGIN x composition error, SUM_DEPTH u s) x the entry's scale."""
    return np.maximum(COMP_MARGIN * np.asarray(comp_err), SUM_DEPTH * U * np.asarray(mag))


# ------------------------------------------------------------------------------------------------------------------ the inputs

def rng(name):
    """The generator of a named input: seeded by the name's crc32, so a case's inputs never depend on what ran before it."""
    return np.random.RandomState(zlib.crc32(name.encode()))


def dy(a, scale=1.0, step=1024.0):
    """float32 multiples of 1 / step (never -0.0)"""
    return (np.round(np.asarray(a, dtype=np.float64) * scale * step) / step + 0.0).astype(np.float32)


def is_dyadic(a, step=1024.0, limit=2.0 ** 13):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.all(np.isfinite(a)) and np.all(a * step == np.round(a * step)) and np.all(np.abs(a) < limit))


# -------------------------------------------------------------------------------------------------------------- the arithmetic

def quotient(num, den):
    """num / den per entry; 0 where both are 0, inf where only den is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))


class Errors:
    """err, cerr, size, mag of one shape -> bound = entry_bound(cerr, mag) and ratio = err / bound beside them."""

    def __init__(self, err, cerr, size, mag):
        self.err, self.cerr, self.size = err, cerr, size
        self.bound = entry_bound(cerr, mag)
        self.ratio = quotient(err, self.bound)

    @property
    def worst(self):
        """the largest error / bound; 0.0 of no entry"""
        return float(self.ratio.max()) if self.ratio.size else 0.0

    @property
    def at(self):
        """the index of the entry with the largest error / bound"""
        return np.unravel_index(int(np.argmax(self.ratio)), self.ratio.shape)

    def row(self):
        """(kernel error, composition error, bound, ratio) of that entry, the first three relative to its own magnitude"""
        i = self.at
        unit = self.size[i] or 1.0
        return self.err[i] / unit, self.cerr[i] / unit, self.bound[i] / unit, self.ratio[i]

    def check(self, *who):
        """No entry over its bound.  Written as ~(err <= bound): a NaN that slipped through fails, it does not pass."""
        bad = np.argwhere(~(self.err <= self.bound))
        assert bad.size == 0, who + ("entries over their bound", len(bad), bad[:8].tolist(), self.worst)


def errors(got, want, mag, comp):
    """Finite float64 arrays of one shape -> Errors.  A non-finite entry of `comp` drops the composition's term of that entry's
    bound: the derived term stands alone.  (A sweep whose composition must be finite asserts that itself.)"""
    with np.errstate(invalid="ignore"):
        cerr = np.where(np.isfinite(comp), np.abs(comp - want), 0.0)
    return Errors(np.abs(got - want), cerr, np.abs(want), mag)


# ------------------------------------------------------------------------------------------------------------------- the table

class Table:
    """The lines a sweep measured in this process, the worst line per key, and their report.  `lines` and `worst` are the
    sweep's TABLE and WORST: a test may read, cut and clear them."""

    def __init__(self, head, env=None):
        self.head, self.env, self.lines, self.worst = head, env, [], {}

    def add(self, line, key=None, ratio=0.0):
        """Appends the line; under a key, keeps it as worst[key] = (ratio, line) where the ratio is the key's largest so far."""
        self.lines.append(line)
        if key is not None and (key not in self.worst or ratio > self.worst[key][0]):
            self.worst[key] = (ratio, line)

    def report(self, since):
        """Prints the head and the lines after `since`; appends those lines to the file the variable `env` names, if it is set."""
        lines = "\n".join(self.lines[since:])
        print(self.head + "\n" + lines)
        path = os.environ.get(self.env) if self.env else None
        if path:
            with open(path, "a") as f:
                f.write(lines + "\n")
