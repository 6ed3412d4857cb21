"""What every ctypes mirror of this package shares: the signature binder, the owner of a library handle and byte buffers as C arrays.
Imports nothing of the package."""
import ctypes as C

import numpy as np


def bind(lib, *tables):
    """Give the functions of `lib` (a CDLL) the signatures of `tables` ({name: (restype, argtypes)}) and return it.  The library object
    itself remembers the tables it holds, so a table is bound once per library and a library met for the first time -- one swapped in behind
    decoder._LIB -- gets every table its callers ask for."""
    held = lib.__dict__.setdefault("_tables_bound", [])
    for sigs in tables:
        if not any(t is sigs for t in held):
            for name, (res, args) in sigs.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            held.append(sigs)
    return lib


class Handle:
    """Owner of one library object: self._h, made by self._lib, given back to the entry point `_destroy` names by close() or when the
    owner goes, once."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


NO_DATA = np.zeros(0, np.uint8)


def as_u8(data):
    if data is None:  # an idle slot (MobiclipBatch.set_idle): a NULL pointer for the library
        return NO_DATA
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    if a.dtype != np.uint8:
        a = a.view(np.uint8)
    return np.ascontiguousarray(a)


def byte_arrays(datas, n):
    """byte buffers (None: no data) -> (the uint8 arrays, to be kept alive over the call; void *[n]; size_t[n])"""
    bufs = [as_u8(d) for d in datas]
    ptrs = (C.c_void_p * n)(*[None if b is NO_DATA else b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[b.size for b in bufs])
    return bufs, ptrs, lens
