"""Physical constants and unit conversions used on the hot path.

Values are the reference's (constants.py:26,29,32,34,37,41,44,50) and must stay bit-identical:
lengths in m, density in g/cm^3, gz in mGal, the gradient tensor in Eotvos, magnetization in A/m, total
field in uT.
"""
#: gravitational constant for density in g/cm^3 (constants.py:34) -- used by prism AND tesseroid gz
G = 0.00000006673
#: SI gravitational constant (constants.py:32) -- not used by gz
Gs = 0.00000000006673
#: m/s^2 -> mGal (constants.py:29)
SI2MGAL = 100000.0
#: mean Earth radius in m (constants.py:44)
MEAN_EARTH_RADIUS = 6378137.0
#: mu_0 / (4 pi) in H/m (constants.py:37)
CM = 10. ** (-7)
#: the reference's tesla conversion (constants.py:41): 10**6, i.e. T -> uT, not the 10**9 (T -> nT) its
#: docstring names.  CM * T2NT == 0.09999999999999999 scales the total-field kernel (gravmag.prism.tf).
T2NT = 10. ** (6)
#: 1/s^2 -> Eotvos (constants.py:26): scales the gravity gradient tensor (G * SI2EOTVOS)
SI2EOTVOS = 1000000000.0
#: gravitational acceleration in m/s^2 (constants.py:50): the geoid is the potential times G / g0
g0 = 9.80
