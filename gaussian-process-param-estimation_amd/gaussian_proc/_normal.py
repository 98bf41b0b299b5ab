"""The standard normals of the device sampler, restated in numpy (HIP-free).

``sample_normal_kernel`` (csrc/gpmi_sample.hip) fills the normals of
``GaussianProcess.sample`` / ``MixedCorrelation.sample`` with a counter-based
generator: entry i of draw j is a function of (seed, j, i) alone,

  key = seed G + j H                                   (mod 2^64)
  x1  = splitmix64(key + 2 i),  x2 = splitmix64(key + 2 i + 1)
  u   = ((x >> 11) + 0.5) 2^-53                        (never zero)
  xi  = sqrt(-2 ln u1) cos(2 pi u2)                    (Box-Muller)

with G = 0x9E3779B97F4A7C15 and H = 0xD1B54A32D192ED03, the constants of the
Rademacher probes (csrc/gpmi_sparse.hip: rademacher_kernel). This module is the
definition the device is tested against, and it lets a user reproduce the xi of a
draw: ``sample(..., seed=s, first=f, size=k)`` is L times the columns of
``standard_normals(s, f, n, k)`` up to the rounding of log, cos and sqrt.
"""

import numpy

__all__ = ['standard_normals']

_G = numpy.uint64(0x9E3779B97F4A7C15)
_H = numpy.uint64(0xD1B54A32D192ED03)
_M1 = numpy.uint64(0xBF58476D1CE4E5B9)
_M2 = numpy.uint64(0x94D049BB133111EB)
_TWO_PI = 6.283185307179586


def _splitmix64(x):
    x = x + _G
    x = (x ^ (x >> numpy.uint64(30))) * _M1
    x = (x ^ (x >> numpy.uint64(27))) * _M2
    return x ^ (x >> numpy.uint64(31))


def _unit(x):
    return ((x >> numpy.uint64(11)).astype(numpy.float64) + 0.5) * 2.0 ** -53


def standard_normals(seed, first, n, size):
    """-> xi (n, size): column k is the draw of global index ``first + k`` under
    ``seed``, row i its entry i. The values depend on (seed, first + k, i) only."""
    seed, first, n, size = int(seed), int(first), int(n), int(size)
    if seed < 0 or first < 0 or n < 0 or size < 0:
        raise ValueError('seed, first, n and size must be non-negative')
    mask = (1 << 64) - 1
    j = numpy.array([(first + k) & mask for k in range(size)], dtype=numpy.uint64)
    i = numpy.arange(n, dtype=numpy.uint64)
    with numpy.errstate(over='ignore'):
        key = numpy.uint64(seed & mask) * _G + j * _H                 # (size,)
        c = key[None, :] + numpy.uint64(2) * i[:, None]               # (n, size)
        u1 = _unit(_splitmix64(c))
        u2 = _unit(_splitmix64(c + numpy.uint64(1)))
    return numpy.sqrt(-2.0 * numpy.log(u1)) * numpy.cos(_TWO_PI * u2)
