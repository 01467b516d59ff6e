"""Plug-in surface of the hot path: the same names the reference exports from models/__init__.py:2-6
for the five in-scope model families, plus BiCut / MOECut / PLECut from the "next" row N4
(section 8f; models/__init__.py:1,7-8), and the probing study's TaskC, TaskR, ProbeBase and Probe."""
from .Bicut import BiCut
from .Choopy import Choopy
from .AttnCut import AttnCut
from .MtChoopy import MtChoopy
from .MtAttnCut import MtAttnCut
from .MMOECut import MMOECut
from .MOECut import MOECut
from .PLECut import PLECut
from .Classification import TaskC
from .Rerank import TaskR
from .Probe import ProbeBase, Probe

__all__ = ["Choopy", "AttnCut", "MtChoopy", "MtAttnCut", "MMOECut", "MOECut", "PLECut", "BiCut", "TaskC", "TaskR", "ProbeBase", "Probe"]
