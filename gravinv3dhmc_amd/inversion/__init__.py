"""Potentials (GravMagModule, JointModule, MultiComponentModule, MagVectorModule,
TesseroidMagVectorModule, TesseroidMultiComponentModule) and sampler (HamitonianMC, HMCSample)."""
from .hmc import HamitonianMC, HMCSample, HMCSampleBatch  # noqa: F401
from .joint import JointModule  # noqa: F401
from .multicomp import MultiComponentModule, TesseroidMultiComponentModule  # noqa: F401
from .magvector import MagVectorModule, TesseroidMagVectorModule  # noqa: F401
from .potential import GravMagModule  # noqa: F401
from .reginv import BootStrap, ConjugateGradient  # noqa: F401
