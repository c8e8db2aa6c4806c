"""Conversions between the reference layout of the SU(3) fields (sites first, the 3 x 3 matrix last) and the native one
(the nine entries of a matrix as planes of V sites), for the tests that hand fields to the native entry points.  Every
function takes and returns numpy arrays or torch tensors alike; the result is contiguous."""
import numpy as np


def _swap(a):
    """the last two axes exchanged"""
    a = a.swapaxes(-1, -2)
    return a.contiguous() if hasattr(a, 'contiguous') else np.ascontiguousarray(a)


def pack(x):
    """x[nb, 4, T, X, Y, Z, 3, 3] (or any site axes) -> the native layout xn[nb, 4, 9, V]"""
    return _swap(x.reshape(x.shape[0], 4, -1, 9))


def unpack(xn, L):
    return _swap(xn).reshape(xn.shape[0], 4, *L, 3, 3)


def pack_g(g):
    """g[nb, T, X, Y, Z, 3, 3] -> gn[nb, 9, V]"""
    return _swap(g.reshape(g.shape[0], -1, 9))


def unpack_g(gn, L):
    return _swap(gn).reshape(gn.shape[0], *L, 3, 3)


def pack_dec(b):
    """a stacked decorated field b[nb, 4, 3, T, X, Y, Z, 3, 3] -> the native layout [nb, 4, 3, 9, V]"""
    return _swap(b.reshape(b.shape[0], 4, 3, -1, 9))


def unpack_dec(bn, L):
    return _swap(bn).reshape(bn.shape[0], 4, 3, *L, 3, 3)
