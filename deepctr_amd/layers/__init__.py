"""In-scope layer classes under the reference's names (deepctr/layers/__init__.py:15-54 lists the full
``custom_objects`` registry; the subset below is what DeepFM / DCN / xDeepFM / DIN and the AFM / PNN
siblings need — SURVEY.md §8a)."""
from .activation import Dice
from .core import DNN, Dense, LocalActivationUnit, PredictionLayer, RegulationModule
from .interaction import (AFMLayer, BiInteractionPooling, BilinearInteraction, BridgeModule, CIN, CrossNet, CrossNetMix, FEFMLayer, FM,
                          FGCNNLayer, FieldWiseBiInteraction, FwFMLayer, InnerProductLayer, InteractingLayer, SENETLayer)
from .normalization import LayerNormalization
from .sequence import AttentionSequencePoolingLayer, BiLSTM, BiasEncoding, DynamicGRU, KMaxPooling, PositionEncoding, SequencePoolingLayer, Transformer, WeightedSequenceLayer
from .utils import Concat, Hash, Linear, NoMask, add_func, combined_dnn_input, concat_func

custom_objects = {
    'DNN': DNN,
    'PredictionLayer': PredictionLayer,
    'FM': FM,
    'AFMLayer': AFMLayer,
    'BiInteractionPooling': BiInteractionPooling,
    'CrossNet': CrossNet,
    'CrossNetMix': CrossNetMix,
    'CIN': CIN,
    'InnerProductLayer': InnerProductLayer,
    'InteractingLayer': InteractingLayer,
    'SENETLayer': SENETLayer,
    'BilinearInteraction': BilinearInteraction,
    'FwFMLayer': FwFMLayer,
    'FEFMLayer': FEFMLayer,
    'FieldWiseBiInteraction': FieldWiseBiInteraction,
    'BridgeModule': BridgeModule,
    'RegulationModule': RegulationModule,
    'LocalActivationUnit': LocalActivationUnit,
    'Dice': Dice,
    'SequencePoolingLayer': SequencePoolingLayer,
    'WeightedSequenceLayer': WeightedSequenceLayer,
    'AttentionSequencePoolingLayer': AttentionSequencePoolingLayer,
    'Transformer': Transformer,
    'PositionEncoding': PositionEncoding,
    'DynamicGRU': DynamicGRU,
    'BiLSTM': BiLSTM,
    'BiasEncoding': BiasEncoding,
    'KMaxPooling': KMaxPooling,
    'FGCNNLayer': FGCNNLayer,
    'LayerNormalization': LayerNormalization,
    'Hash': Hash,
    'Linear': Linear,
    'Concat': Concat,
    'NoMask': NoMask,
}
