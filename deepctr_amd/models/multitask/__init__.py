"""The multi-task models of ``deepctr.models.multitask``: SharedBottom, ESMM, MMOE, PLE."""
from .esmm import ESMM
from .mmoe import MMOE
from .ple import PLE
from .sharedbottom import SharedBottom
from ._base import MultiTaskModel

__all__ = ["SharedBottom", "ESMM", "MMOE", "PLE", "MultiTaskModel"]
