"""Drop-in `vqa.models` package of the MI355X NeuralCX path: the VQA-model plugin surface the counterexample scorer needs
(`factory(opt, vocab_words, vocab_answers, cuda, data_parallel)`, `model_names`, the MUTAN and MLB no-attention models, the MLB
attention model) plus, in
`vqa.models.cx`, the NeuralModel / baseline scorers whose hot path runs in libneuralcx_hip.so."""
from . import att, cx, fusion, noatt, seq2vec, utils

MutanNoAtt = noatt.MutanNoAtt
MLBNoAtt = noatt.MLBNoAtt
MLBAtt = att.MLBAtt
MLBFusion = fusion.MLBFusion
factory = utils.factory
model_names = utils.model_names

__all__ = ["MutanNoAtt", "MLBNoAtt", "MLBAtt", "MLBFusion", "factory", "model_names", "att", "cx", "fusion", "noatt", "seq2vec", "utils"]
