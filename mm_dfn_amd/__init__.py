"""mm_dfn_amd: MI355X-native (gfx950) implementation of the MM-DFN hot path.

Drop-in ``nn.Module`` counterparts of the reference's GraphConvolution /
GCNII_lyc (model_GCN.py), MM_GCN / MM_GCN2 (model_mm.py), DialogueGNNModel (model.py) and
FocalLoss (loss.py) whose compute is hand-written HIP behind a C ABI
(include/mmdfn_hip.h).  See DESIGN.md.
"""
from .layout import DialogueLayout, BlockTileAdjacency  # noqa: F401
from .graph_conv import GraphConvolution, GCNII_lyc, GCNII  # noqa: F401
from .mm_gcn import MM_GCN  # noqa: F401
from .mm_gcn2 import MM_GCN2  # noqa: F401
from .dialogue_model import DialogueGNNModel  # noqa: F401
from .loss import FocalLoss, NLLLoss, MaskedNLLLoss  # noqa: F401
from .fusion import MFN, MMGatedAttention  # noqa: F401
from .multistream import MultiStreamGraphModel  # noqa: F401
from .attention import MatchingAttention  # noqa: F401
from .dialogue_rnn import DialogueRNN  # noqa: F401
from .recurrent_models import GRUModel, LSTMModel, DialogRNNModel  # noqa: F401
from .cnn_features import CNNFeatureExtractor  # noqa: F401
