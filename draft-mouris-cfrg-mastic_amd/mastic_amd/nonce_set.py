"""Replay protection: the nonces an aggregator has admitted, resident in HBM
(``mastic_nonce_set_*`` in ``include/mastic_hip.h``).

The reference's driver (poc/examples.py) handles 13 reports and has no replay
handling; an aggregator that holds millions of reports on the GPU has to
drop a report whose nonce it has seen, without the nonces leaving HBM.
"""
import ctypes

import numpy as np

from . import _lib
from .vdaf import Reports, _check


class NonceSet:
    """A set of 16-byte nonces on ``mastic``'s GPU.

    ``admit`` of a batch returns, per nonce, 1 iff it was not in the set and
    does not occur earlier in the batch, and adds the batch to the set.  The
    mask depends on the set's contents and the batch only (not on
    ``hash_key``, the 16-byte secret of the table's keyed hash; None draws it
    from the operating system).  ``capacity`` sizes the set up front.  The
    set keeps ``mastic`` alive and must not outlive its context."""

    def __init__(self, mastic, capacity: int = 0, hash_key: bytes = None):
        if hash_key is not None and len(hash_key) != 16:
            raise ValueError("hash_key must be 16 bytes")
        self._m = mastic
        self._ptr = ctypes.c_void_p()
        _check(mastic._ctx, _lib.lib().mastic_nonce_set_create(mastic._ctx, int(capacity), hash_key,
                                                               ctypes.byref(self._ptr)))

    def __del__(self):
        if getattr(self, "_ptr", None) and getattr(self._m, "_ctx", None):
            _lib.lib().mastic_nonce_set_destroy(self._ptr)
        self._ptr = None

    def __len__(self):
        return _lib.lib().mastic_nonce_set_count(self._ptr)

    @staticmethod
    def _nonces(data):
        data = bytes(data)
        if len(data) % 16:
            raise ValueError("nonces must be a multiple of 16 bytes")
        return (data, len(data) // 16)

    def admit(self, x):
        """``x``: a resident :class:`Reports` batch or view (its nonces are read
        in HBM) or the concatenated nonces as bytes.  Returns the fresh mask
        (``np.uint8``, one per nonce)."""
        if isinstance(x, Reports):
            fresh = np.empty(x.n, np.uint8)
            _check(self._m._ctx, _lib.lib().mastic_nonce_set_admit_reports(self._ptr, x._ptr, _lib.buf(fresh), None))
            return fresh
        (data, n) = self._nonces(x)
        fresh = np.empty(n, np.uint8)
        _check(self._m._ctx, _lib.lib().mastic_nonce_set_admit(self._ptr, _lib.buf(data), n, _lib.buf(fresh), None))
        return fresh

    def contains(self, nonces):
        """Per nonce of ``nonces`` (bytes): 1 iff it is in the set.  Inserts nothing."""
        (data, n) = self._nonces(nonces)
        found = np.empty(n, np.uint8)
        _check(self._m._ctx, _lib.lib().mastic_nonce_set_contains(self._ptr, _lib.buf(data), n, _lib.buf(found)))
        return found

    def export(self) -> bytes:
        """The set's nonces, concatenated, in no specified order (a checkpoint)."""
        out = np.empty(16 * len(self), np.uint8)
        n = ctypes.c_size_t()
        _check(self._m._ctx, _lib.lib().mastic_nonce_set_export(self._ptr, _lib.buf(out), len(out) // 16,
                                                                ctypes.byref(n)))
        return out[:16 * n.value].tobytes()

    def load(self, data):
        """Restore a checkpoint: admit ``export()``'s bytes.  Returns the number added."""
        before = len(self)
        self.admit(data)
        return len(self) - before
