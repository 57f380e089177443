"""Host reference and table helpers shared by the join-kind tests (a plain
module, not a conftest): host columns with optional validity, their device
copies as nullable column descriptors, output tables as sorted row tuples with
None for a null cell, and a dict-based reference join of every kind with
null == null (None == None as a dict key)."""
from collections import defaultdict

import numpy as np

INNER, LEFT, LEFT_SEMI, LEFT_ANTI = 0, 1, 2, 3
KINDS = {"inner": INNER, "left": LEFT, "semi": LEFT_SEMI, "anti": LEFT_ANTI}


class Col:
    """Host column: values (numpy array, or list of bytes for STRING), valid
    (bool array, or None = no mask)."""

    def __init__(self, type_id, values, valid=None):
        self.type_id = type_id
        self.values = values
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)

    def __len__(self):
        return len(self.values)

    def cell(self, i):
        if self.valid is not None and not self.valid[i]:
            return None
        v = self.values[i]
        return v if isinstance(v, bytes) else v.item()

    def head(self, n):
        return Col(self.type_id, self.values[:n], None if self.valid is None else self.valid[:n])


class Dev:
    """Device copy of a list of Col; .cols are the nullable descriptors."""

    def __init__(self, dj, cols):
        self.dj = dj
        self.cols, self._fixed, self._raw, self._masks = [], [], [], []
        for c in cols:
            if c.type_id == dj.TYPE_STRING:
                off, ch, nb = dj.upload_strings(list(c.values))
                self._raw += [off, ch]
                desc = (dj.TYPE_STRING, off, ch, nb)
            else:
                d = dj.upload_column(np.asarray(c.values), c.type_id)
                self._fixed.append(d)
                desc = d.desc
            if c.valid is None:
                self.cols.append(desc)
            else:
                m = dj.upload_mask(c.valid)
                self._masks.append(m)
                self.cols.append(desc + (m,))

    def free(self):
        for d in self._fixed + self._masks:
            d.free()
        for p in self._raw:
            self.dj.lib().dj_dfree(p)


def decode(col):
    off, ch = col
    raw = ch.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def row_key(row):
    """Total order over rows whose cells are None, bytes or numbers."""
    return tuple((0, b"", 0) if x is None else
                 ((1, x, 0) if isinstance(x, bytes) else (2, b"", x)) for x in row)


def rows(cols, masks):
    """Output table -> sorted list of row tuples, None for a null cell."""
    lists = []
    for c, m in zip(cols, masks):
        vals = decode(c) if isinstance(c, tuple) else c.tolist()
        if m is not None:
            vals = [v if ok else None for v, ok in zip(vals, m)]
        lists.append(vals)
    n = len(lists[0]) if lists else 0
    return sorted((tuple(l[i] for l in lists) for i in range(n)), key=row_key)


def host_rows(table):
    n = len(table[0]) if table else 0
    return [tuple(c.cell(i) for c in table) for i in range(n)]


def ref_join(kind, left, right, lon, ron):
    """Join of the given kind over lists of Col; sorted rows. A LEFT join's
    unmatched rows carry None in every right-hand cell."""
    lrows, rrows = host_rows(left), host_rows(right)
    index = defaultdict(list)
    for j, row in enumerate(rrows):
        index[tuple(row[c] for c in ron)].append(j)
    out = []
    pad = (None,) * len(right)
    for row in lrows:
        hits = index.get(tuple(row[c] for c in lon), ())
        if kind == INNER:
            out += [row + rrows[j] for j in hits]
        elif kind == LEFT:
            out += [row + rrows[j] for j in hits] if hits else [row + pad]
        elif kind == LEFT_SEMI:
            out += [row] if hits else []
        elif kind == LEFT_ANTI:
            out += [] if hits else [row]
        else:
            raise ValueError(kind)
    return sorted(out, key=row_key)


def run_join(dj, comm, kind, left, right, lon, ron, over_decom=1):
    """The library's join of the given kind on one rank -> (cols, masks)."""
    dl, dr = Dev(dj, left), Dev(dj, right)
    try:
        return dj.cpp_distributed_join_ncols_multi(
            comm, kind, dl.cols, len(left[0]), dr.cols, len(right[0]), lon, ron, over_decom)
    finally:
        dl.free()
        dr.free()


def check_masks(kind, left, right, cols, masks):
    """Mask presence by the kind's rule; returns the number of output rows.
    (Exact null counts are checked against the masks when the table is read
    back, distributed_join_amd.table_to_numpy_nullable.)"""
    ncols = len(left) + (len(right) if kind in (INNER, LEFT) else 0)
    assert len(cols) == ncols and len(masks) == ncols
    for m, c in zip(masks, left):
        assert (m is not None) == (c.valid is not None)
    for m, c in zip(masks[len(left):], right):
        if kind == LEFT:
            assert m is not None
        else:
            assert (m is not None) == (c.valid is not None)
    c0 = cols[0]
    return len(c0[0]) - 1 if isinstance(c0, tuple) else len(c0)
