"""Shared helpers of the prism / tesseroid front-ends."""
import numpy as np


def active_cells(model, dens):
    """Bounds table (M, 6) and density vector (M) of the cells a reference loop would visit.

    Mirrors the skipping rule of gravmag/prism.py:299-301 and gravmag/tesseroid.py:95-98,
    126-153: a cell is skipped when it is None (carved) or when it has no 'density' property
    and no `dens` override is given."""
    props = getattr(model, "props", None)
    if hasattr(model, "cell_bounds") and hasattr(model, "active_index"):
        if dens is None and (props is None or "density" not in props):
            return np.zeros((0, 6)), np.zeros(0), None
        bounds = model.cell_bounds(active_only=True)
        idx = model.active_index()
        if dens is not None:
            rho = np.full(len(idx), float(dens))
        else:
            rho = np.asarray(props["density"], dtype=np.float64)[idx]
        return bounds, rho, idx
    rows, rho = [], []
    for cell in model:
        if cell is None or ("density" not in cell.props and dens is None):
            continue
        rows.append(cell.get_bounds())
        rho.append(float(dens) if dens is not None else float(cell.props["density"]))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6), np.asarray(rho, dtype=np.float64), None



def _mag_vector(m, f):
    """(mx, my, mz) of one magnetization value: a scalar is an intensity along the field direction f
    (prism.py:665-733 multiplies it by dircos(inc, dec)), anything else the vector itself."""
    if np.ndim(m) == 0:
        return (m * f[0], m * f[1], m * f[2])
    mx, my, mz = m
    return (mx, my, mz)


def active_cells_mag(model, pmag, f):
    """Bounds table (M, 6), magnetization table (M, 3) in A/m and, for a mesh, the flat indices of the
    cells the reference's magnetic loop would visit; f is the field direction dircos(inc, dec).

    The magnetic analogue of `active_cells` (gravmag/prism.py:1140-1160, 665-733): a cell is skipped
    when it is None (carved) or when it has no 'magnetization' property and `pmag` is None.  `pmag`
    (a vector, or a scalar intensity along f) replaces every cell's property; so does a cell's scalar
    'magnetization' (times f).  On a mesh the rule and the table are evaluated for all cells at once."""
    props = getattr(model, "props", None)
    fixed = None if pmag is None else np.asarray(_mag_vector(pmag, f), dtype=np.float64)
    if hasattr(model, "cell_bounds") and hasattr(model, "active_index"):
        if pmag is None and (props is None or "magnetization" not in props):
            return np.zeros((0, 6)), np.zeros((0, 3)), None
        bounds = model.cell_bounds(active_only=True)
        idx = model.active_index()
        if fixed is not None:
            return bounds, np.tile(fixed, (len(idx), 1)), idx
        mag = np.asarray(props["magnetization"], dtype=np.float64)[idx]
        if mag.ndim == 1:                  # one intensity per cell, along the field
            mag = np.stack([mag * f[0], mag * f[1], mag * f[2]], axis=1)
        return bounds, np.ascontiguousarray(mag.reshape(len(idx), 3)), idx
    rows, mags = [], []
    for cell in model:
        if cell is None or ("magnetization" not in cell.props and pmag is None):
            continue
        rows.append(cell.get_bounds())
        mags.append(fixed if fixed is not None else _mag_vector(cell.props["magnetization"], f))
    return (np.asarray(rows, dtype=np.float64).reshape(-1, 6), np.asarray(mags, dtype=np.float64).reshape(-1, 3),
            None)
