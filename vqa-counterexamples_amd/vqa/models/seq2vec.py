"""Question encoders.  The reference uses skipthoughts.BayesianUniSkip (GRU 620 -> 2400) from an un-vendored
submodule that needs downloaded tables (vqa/models/seq2vec.py:79-85); offline we provide a GRU encoder with the
same interface (wids[B, T] right-padded with 0 -> [B, dim_q]).  It is an INPUT producer of the hot path.
The reference's other working encoder, `2-lstm` (TwoLSTM, vqa/models/seq2vec.py:48-76), is written out in full there and is TwoLSTM here."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class GRUEncoder(nn.Module):
    """nn.Embedding -> nn.GRU -> the hidden state after the last word.  On a CUDA device, when no gradient can be wanted and dropout
    is inert, forward runs in the HIP library (ops.gru_encode: padded steps are skipped); `use_hip = False` keeps it in PyTorch.
    `use_hip_train = True` (off by default) also trains it there: a CUDA fp32 module called with grad mode on and a parameter that
    requires grad runs neuralcx.vqa_train.GruTrainFunction (forward with a stash, backward through time); its dropout stays in torch.
    `hip_x6` is handed to both HIP routes and changes no routing decision: None = the process-wide choice (ops.EXTRA_FLAGS, NCX_X6=1),
    True / False = the bf16 x 6 / the fp32 form of the step kernel (ops.gru_step_form; train.py --x6_seq2vec sets True) and, on the
    training route, of the backward's matrix products that have one (ops.gru_bwd_form)."""
    use_hip = True
    use_hip_train = False
    hip_x6 = None

    def __init__(self, vocab_words, dim_q=2400, dim_emb=620, dropout=0.25):
        super().__init__()
        self.embedding = nn.Embedding(len(vocab_words) + 1, dim_emb, padding_idx=0)
        self.gru = nn.GRU(dim_emb, dim_q, batch_first=True)
        self.dropout = nn.Dropout(dropout)

    def _hip_ok(self, wids):
        if not (self.use_hip and wids.is_cuda and wids.dim() == 2 and 1 <= wids.shape[1] <= 64 and wids.shape[0] >= 1):
            return False
        if self.training and self.dropout.p > 0:
            return False
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return False
        return all(p.dtype == torch.float32 and p.device == wids.device for p in params)

    def _hip_weights(self):
        """ops.GruWeights of the current parameters; repacked when a parameter moved or was written to (load_state_dict, .to(),
        an optimizer step) -- data_ptr and the in-place version counter of every parameter are the key."""
        from neuralcx import ops
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        hit = self.__dict__.get("_hip_gru")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_hip_gru"] = (key, ops.gru_weights(self))
        return hit[1]

    def drop_hip_weights(self):
        self.__dict__.pop("_hip_gru", None)
        self.__dict__.pop("_hip_gru_train", None)

    def _hip_train_ok(self, wids):
        if not (self.use_hip_train and wids.is_cuda and wids.dim() == 2 and 1 <= wids.shape[1] <= 64 and wids.shape[0] >= 1):
            return False
        params = list(self.parameters())
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
            return False
        return all(p.dtype == torch.float32 and p.device == wids.device for p in params)

    def forward(self, wids):
        if self._hip_ok(wids):
            from neuralcx import ops
            return ops.gru_encode(wids, self._hip_weights(), x6=self.hip_x6)
        if self._hip_train_ok(wids):
            from neuralcx.vqa_train import GruTrainFunction
            g = self.gru
            return self.dropout(GruTrainFunction.apply(wids, self.embedding.weight, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, self))
        x = self.embedding(wids)
        out, _ = self.gru(x)
        last = (wids > 0).sum(1).clamp(min=1) - 1            # last valid step (right padding)
        return self.dropout(out[torch.arange(wids.shape[0], device=wids.device), last])


class TwoLSTM(nn.Module):
    """The reference's TwoLSTM (vqa/models/seq2vec.py:48-76): tanh(nn.Embedding) -> rnn_0 = LSTM(emb_size -> H) -> rnn_1 = LSTM(H -> H);
    the output is [vec_0 | vec_1] of shape [B, 2 H], each layer's output at the row's last step, dropout p = 0.3 on both in training.
    Lengths as process_lengths + select_last (seq2vec.py:11-25): len_b = T - #{t : wids[b, t] == 0}, the selected step is len_b - 1,
    which for an all-padding row is index -1, step T - 1 (GRUEncoder clamps to step 0 instead).  state_dict names and shapes are the
    reference's, so its `2-lstm` checkpoints load.

    One deliberate difference: the reference builds both nn.LSTMs WITHOUT batch_first and feeds them [B, T, emb], so as written its
    recurrence runs over the batch axis and a question's vector depends on its place in the batch (the same question at batch
    positions 2 and 1 differs by 0.18; alone at position 0 against position 1 by 0.07).  This class is the intended model: recurrence
    over time, batch_first=True; that flag changes no parameter name or shape.

    On a CUDA device in eval mode, when no gradient can be wanted, forward runs in the HIP library (ops.lstm_encode: padded steps are
    skipped, the two layers run as a wavefront); `use_hip = False` keeps it in PyTorch.  It trains under torch autograd, unless
    `use_hip_bptt = True` (off by default; train.py --hip_2lstm_train): then a CUDA fp32 module called with grad mode on and a parameter
    that requires grad runs neuralcx.vqa_train.LstmTrainFunction (forward with a stash, backward through time); its dropout stays in
    torch, on the two halves in the torch path's order.
    `hip_x6` is handed to both HIP routes and changes no routing decision: None = the process-wide choice (ops.EXTRA_FLAGS, NCX_X6=1),
    True / False = the bf16 x 6 / the fp32 form of the step kernel (ops.lstm_step_form; train.py --x6_2lstm sets True)."""
    use_hip = True
    use_hip_bptt = False
    hip_x6 = None
    p_drop = 0.3

    def __init__(self, vocab_words, emb_size, hidden_size):
        super().__init__()
        self.emb_size, self.hidden_size = emb_size, hidden_size
        self.embedding = nn.Embedding(len(vocab_words) + 1, emb_size, padding_idx=0)
        self.rnn_0 = nn.LSTM(emb_size, hidden_size, num_layers=1, batch_first=True)
        self.rnn_1 = nn.LSTM(hidden_size, hidden_size, num_layers=1, batch_first=True)

    def _hip_ok(self, wids):
        if not (self.use_hip and wids.is_cuda and wids.dim() == 2 and 1 <= wids.shape[1] <= 64 and wids.shape[0] >= 1):
            return False
        if self.training:                                        # p = 0.3 is fixed: dropout is live
            return False
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return False
        return all(p.dtype == torch.float32 and p.device == wids.device for p in params)

    def _hip_weights(self):
        """ops.LstmWeights of the current parameters; repacked when a parameter moved or was written to (GRUEncoder's key)."""
        from neuralcx import ops
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        hit = self.__dict__.get("_hip_lstm")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_hip_lstm"] = (key, ops.lstm_weights(self))
        return hit[1]

    def drop_hip_weights(self):
        self.__dict__.pop("_hip_lstm", None)
        self.__dict__.pop("_hip_lstm_train", None)

    def _hip_bptt_ok(self, wids):
        if not (self.use_hip_bptt and wids.is_cuda and wids.dim() == 2 and 1 <= wids.shape[1] <= 64 and wids.shape[0] >= 1):
            return False
        params = list(self.parameters())
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
            return False
        return all(p.dtype == torch.float32 and p.device == wids.device for p in params)

    def forward(self, wids):
        if self._hip_ok(wids):
            from neuralcx import ops
            return ops.lstm_encode(wids, self._hip_weights(), x6=self.hip_x6)
        if self._hip_bptt_ok(wids):
            from neuralcx.vqa_train import LstmTrainFunction
            r0, r1, H = self.rnn_0, self.rnn_1, self.hidden_size
            q = LstmTrainFunction.apply(wids, self.embedding.weight, r0.weight_ih_l0, r0.weight_hh_l0, r0.bias_ih_l0, r0.bias_hh_l0,
                                        r1.weight_ih_l0, r1.weight_hh_l0, r1.bias_ih_l0, r1.bias_hh_l0, self)
            # each half as a contiguous [B, H] tensor, vec_0 first: under one seed the masks are the torch path's
            vec_0 = F.dropout(q[:, :H].contiguous(), p=self.p_drop, training=self.training)
            vec_1 = F.dropout(q[:, H:].contiguous(), p=self.p_drop, training=self.training)
            return torch.cat((vec_0, vec_1), 1)
        B, T = wids.shape
        n = (wids != 0).sum(1)
        last = torch.where(n > 0, n, torch.full_like(n, T)) - 1  # select_last's index len - 1; -1 is step T - 1
        rows = torch.arange(B, device=wids.device)
        x = torch.tanh(self.embedding(wids))
        x_0, _ = self.rnn_0(x)
        x_1, _ = self.rnn_1(x_0)
        vec_0 = F.dropout(x_0[rows, last], p=self.p_drop, training=self.training)
        vec_1 = F.dropout(x_1[rows, last], p=self.p_drop, training=self.training)
        return torch.cat((vec_0, vec_1), 1)


def factory(vocab_words, opt, dim_q=2400):
    arch = opt.get("arch", "skipthoughts")
    if arch == "skipthoughts":
        try:
            import skipthoughts                      # optional: the real encoder when the submodule is present
            return getattr(skipthoughts, opt["type"])(opt["dir_st"], vocab_words, dropout=opt["dropout"],
                                                      fixed_emb=opt["fixed_emb"])
        except ImportError:
            return GRUEncoder(vocab_words, dim_q=dim_q, dropout=opt.get("dropout", 0.25))
    if arch == "2-lstm" and "hidden_size" in opt:                # the reference's branch (seq2vec.py:86-89): it reads both keys
        if 2 * opt["hidden_size"] != dim_q:
            raise ValueError("seq2vec 2-lstm: 2 * hidden_size = %d, but the model's dim_q is %d" % (2 * opt["hidden_size"], dim_q))
        return TwoLSTM(vocab_words, opt["emb_size"], opt["hidden_size"])
    if arch in ("gru", "lstm", "2-lstm"):
        return GRUEncoder(vocab_words, dim_q=dim_q, dim_emb=opt.get("emb_size", 620), dropout=opt.get("dropout", 0.0))
    raise NotImplementedError(arch)
