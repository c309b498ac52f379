"""No-attention VQA models used as the frozen feature producer of NeuralCX (reference: vqa/models/noatt.py:9-58).
Exposes what vqa.models.cx needs: .seq2vec, ._fusion(v, q), ._classif(z), .opt['fusion'], .vocab_answers."""
import torch.nn as nn
import torch.nn.functional as F

from . import fusion, seq2vec


class AbstractNoAtt(nn.Module):
    """seq2vec + a fusion (set by the subclass) + the classifier over fusion.dim_h (reference noatt.py:9-35)."""

    def __init__(self, opt=None, vocab_words=(), vocab_answers=()):
        super().__init__()
        opt = opt or {}
        self.opt, self.vocab_words, self.vocab_answers = opt, vocab_words, vocab_answers
        self.num_classes = len(vocab_answers)
        self.seq2vec = seq2vec.factory(vocab_words, opt["seq2vec"], dim_q=opt["fusion"].get("dim_q", 2400))
        self.linear_classif = nn.Linear(opt["fusion"]["dim_h"], self.num_classes)

    def _fusion(self, input_v, input_q):
        return self.fusion(input_v, input_q)

    def _classif(self, x):
        if "activation" in self.opt["classif"]:
            x = getattr(F, self.opt["classif"]["activation"])(x)
        x = F.dropout(x, p=self.opt["classif"]["dropout"], training=self.training)
        return self.linear_classif(x)

    def forward(self, input_v, input_q):
        return self._classif(self._fusion(input_v, self.seq2vec(input_q)))


class MutanNoAtt(AbstractNoAtt):
    """`use_hip_train = True` (set by a caller; never by default) routes forward's fusion + classifier through the HIP library's
    differentiable step (neuralcx.vqa_train.MutanTrainFunction) when the input is a dense [B, dim_v] CUDA tensor and the options
    are the supported model; seq2vec stays in PyTorch and trains under autograd."""
    use_hip_train = False

    def __init__(self, opt=None, vocab_words=(), vocab_answers=()):
        opt = opt or {}
        opt["fusion"]["dim_h"] = opt["fusion"]["dim_mm"]
        super().__init__(opt, vocab_words, vocab_answers)
        self.fusion = fusion.MutanFusion(opt["fusion"])

    def forward(self, input_v, input_q):
        if self.use_hip_train and input_v.is_cuda and input_v.dim() == 2:
            from neuralcx import vqa_train
            if vqa_train.route_for(self.opt) == "hip":
                return vqa_train.module_forward(self, input_v, self.seq2vec(input_q))
        return super().forward(input_v, input_q)


class MLBNoAtt(AbstractNoAtt):
    """The reference's MLBNoAtt (vqa/models/noatt.py:38-46): MLBFusion + (classif.activation) + linear_classif over fusion.dim_h.
    state_dict keys: seq2vec.*, linear_classif.*, fusion.linear_v.*, fusion.linear_q.*.
    `use_hip_train = True` (set by a caller; never by default) routes forward's fusion + classifier through
    neuralcx.vqa_train.MlbTrainFunction under the conditions of MutanNoAtt.forward."""
    use_hip_train = False

    def __init__(self, opt=None, vocab_words=(), vocab_answers=()):
        super().__init__(opt, vocab_words, vocab_answers)
        self.fusion = fusion.MLBFusion(self.opt["fusion"])

    def forward(self, input_v, input_q):
        if self.use_hip_train and input_v.is_cuda and input_v.dim() == 2:
            from neuralcx import vqa_train
            if vqa_train.mlb_route_for(self.opt) == "hip":
                return vqa_train.mlb_module_forward(self, input_v, self.seq2vec(input_q))
        return super().forward(input_v, input_q)
