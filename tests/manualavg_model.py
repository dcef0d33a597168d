"""The specification of manual averaging (include/fdoct_manualavg.h) in NumPy, in doubles: BscanFFT.cpp:1399-1444 restated image
by image.

State: `acc`, an image of doubles that starts at zero (manualaccum, main:933), and `accumulated`, 0 (manualaccumcount, main:567).
m = manualaverages >= 1.  For every linear B-scan, in order:
  REFERENCE   while accumulated < m (1401-1414): acc += bscan; accumulated += 1
              otherwise (1416-1444): emit acc / m, acc = 0, accumulated = 0 -- and the B-scan that arrived is dropped
  KEEP_ALL    acc += bscan; accumulated += 1; as soon as accumulated >= m: emit acc / m, acc = 0, accumulated = 0
An emission is mean = (acc / m).astype(float32) and db = (20.0 * np.log(acc / m) / 2.303).astype(float32) (1419-1423); a mean of
zero gives -inf, as ln does.  `plan` is the same walk without images.
"""
import numpy as np

REFERENCE, KEEP_ALL = 0, 1


def _step(m, mode, accumulated):
    """One image: (it is added, an emission follows, accumulated afterwards)."""
    if mode == REFERENCE:
        return (True, False, accumulated + 1) if accumulated < m else (False, True, 0)
    return (True, True, 0) if accumulated + 1 >= m else (True, False, accumulated + 1)


def plan(m, mode, accumulated, nbscans):
    """(emitted, accumulated afterwards) of nbscans more images."""
    if m < 1 or mode not in (REFERENCE, KEEP_ALL) or not 0 <= accumulated <= m or nbscans < 0:
        raise ValueError("bad arguments")
    emitted = 0
    for _ in range(nbscans):
        _, emit, accumulated = _step(m, mode, accumulated)
        emitted += emit
    return emitted, accumulated


class ManualAvg:
    def __init__(self, manualaverages, count, mode=REFERENCE):
        if manualaverages < 1 or count < 1 or mode not in (REFERENCE, KEEP_ALL):
            raise ValueError("bad arguments")
        self.m, self.count, self.mode = int(manualaverages), int(count), mode
        self.acc = np.zeros(self.count, np.float64)
        self.accumulated = 0

    def add(self, bscans):
        """bscans: float32 (nbscans, ...) images of `count` floats -> (mean, db), float32 (emitted,) + the image's shape."""
        a = np.asarray(bscans, np.float32)
        shape = a.shape[1:]
        a = a.reshape(a.shape[0], self.count)
        means, dbs = [], []
        for img in a:
            add, emit, self.accumulated = _step(self.m, self.mode, self.accumulated)
            if add:
                self.acc += img.astype(np.float64)
            if emit:
                q = self.acc / float(self.m)
                means.append(q.astype(np.float32))
                with np.errstate(divide="ignore", invalid="ignore"):
                    dbs.append((20.0 * np.log(q) / 2.303).astype(np.float32))
                self.acc = np.zeros(self.count, np.float64)
        out_shape = (len(means),) + shape
        return (np.array(means, np.float32).reshape(out_shape), np.array(dbs, np.float32).reshape(out_shape))
