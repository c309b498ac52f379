"""Counterexample models -- drop-in for the reference's vqa/models/cx.py plugin surface.

`NeuralModel` keeps the reference's constructor (cx.py:220-224), `forward(image_features, question_wids,
answer_aids) -> scores[B, K]` (cx.py:261), the mutable `knn_size` attribute, `vqa_forward` (cx.py:64-104) and
the state_dict keys (`answer_embedding.weight`, `linear_1.*`, `linear_2.*`, `linear_3.*`, `out.*`,
`vqa_model.*`; linear_1.weight keeps the concat column order of cx.py:309-320), so checkpoints and calling
code are interchangeable.  Everything below `vqa_forward` -- the answer-embedding products, the 24-way feature
synthesis/concat, the Linear+ReLU+Dropout stack, `out`, and the whole backward -- runs in the HIP library
(libneuralcx_hip.so) through `neuralcx.ops.NeuralCXFunction`.  There is no PyTorch fallback for that part:
on a machine without the library or without a GPU `forward` raises.  `SemanticBaseline` (cx.py:159-210) keeps the
reference's surface likewise; its cosine Gram and scorer run in the same library (see its docstring).  `LinearContext`
(cx.py:139-156) and `PairwiseLinearModel` (cx.py:379-425) keep the reference's constructor, submodule names and state_dict
keys; their forward and backward run in the library through an autograd.Function, so the reference's loop with
torch.optim.Adam trains them.  `ContrastiveModel` (cx.py:428-487), the model of the reference's second script contrastive.py, likewise.
`SimilarityModel` (cx.py:490-518) has no parameters: its scorer is one HIP launch per batch (see its docstring).  Every name the
reference's counterexamples.py imports from this module (counterexamples.py:30-32) exists here; `PairwiseModel` (cx.py:336-376) is
the one without an implementation: its constructor raises.

Deliberate differences from the reference (all supersets):
  * knn_size may be 1..64 (the reference asserts == 24, cx.py:226); config 5 of BASELINE.json uses 48;
  * `trainable_vqa=True` is rejected (input gradients are not produced; the reference's default and every
    options/cx/*.yaml use a frozen VQA model, cx.py:73-80);
  * lesion combination q_emb=z_emb=False with a_emb=True raises a clear error (NameError in the reference);
  * an answer id outside [0, ans_size) raises IndexError like nn.Embedding (cx.py:280), but by default NOT at the offending
    call: the verdict is read without a host sync and surfaces at the next point that syncs anyway -- the next forward
    whose flag copy has landed, `train()` / `eval()` (the reference switches modes around every evaluation and epoch),
    `state_dict()` (every checkpoint save), or `check_answer_ids()`.  `strict_ids=True` (constructor keyword or attribute)
    restores the immediate raise at the price of one host sync per forward; on a CPU device the check is always immediate.
"""
import numpy as np
import torch
import torch.nn as nn

from neuralcx import ops

from .fusion import out_dim as fusion_out_dim

DIM_A = 2400      # cx.py:235


class RandomBaseline(nn.Module):
    """Uniform random scores: Recall@k ~ k / knn_size (reference cx.py:20-30; README 4.20 / 20.85)."""

    def __init__(self, knn_size):
        super().__init__()
        self.knn_size = knn_size

    def forward(self, image_features, question_wids, answer_aids):
        return torch.rand(image_features.size(0), self.knn_size, device=image_features.device)


class DistanceBaseline(nn.Module):
    """Scores knn_size-1 .. 0 for every row: Recall@k == fraction with knn_index < k (reference cx.py:33-44)."""

    def __init__(self, knn_size):
        super().__init__()
        self.knn_size = knn_size

    def forward(self, image_features, question_wids, answer_aids):
        s = torch.arange(self.knn_size - 1, -1, -1, dtype=torch.float32, device=image_features.device)
        return s.view(1, -1).expand(image_features.size(0), self.knn_size).contiguous()


class CXModelBase(nn.Module):
    def __init__(self, vqa_model, knn_size, trainable_vqa=False):
        super().__init__()
        self.vqa_model = vqa_model
        self.trainable_vqa = trainable_vqa
        if vqa_model is not None and not trainable_vqa:
            self.vqa_model.eval()
        self.knn_size = knn_size

    def _hip_vqa_ok(self, image_features):
        from .noatt import MLBNoAtt, MutanNoAtt
        return (isinstance(self.vqa_model, (MutanNoAtt, MLBNoAtt)) and image_features.is_cuda and not self.trainable_vqa
                and getattr(self, "use_hip_vqa", True))

    @torch.no_grad()
    def vqa_forward(self, image_features, question_wids):
        """Frozen VQA model on the original + K candidate images -> a_orig, z_orig, a_knns, z_knns, q_emb
        (same outputs as cx.py:64-104).  For MutanNoAtt and MLBNoAtt on the GPU everything below the question encoder runs in
        the HIP library (ncx_vqa_forward: gather + linear_v + tanh, R-term fusion folded in one chained GEMM,
        classifier; ncx_mlb_forward: gather + linear_v + tanh + hadamard product in one launch, classifier); otherwise plain
        PyTorch (also with use_hip_vqa = False).  Either way the question branch is computed once per question
        (the reference duplicates q K+1 times first, cx.py:83-87)."""
        assert image_features.size(1) == self.knn_size + 1
        B, K1 = image_features.size(0), self.knn_size + 1
        vqa = self.vqa_model
        vqa.eval()
        q_emb = vqa.seq2vec(question_wids)
        if self._hip_vqa_ok(image_features):
            a_o, z_o, a_k, z_k = self._hip_vqa_forward(image_features, q_emb, want_a_orig=True)
            return a_o, z_o, a_k, z_k, q_emb
        v = image_features.reshape(B * K1, -1)
        q_dup = q_emb.view(B, 1, -1).expand(B, K1, q_emb.size(-1)).reshape(B * K1, -1)
        z = vqa._fusion(v, q_dup)
        a = vqa._classif(z)
        a, z = a.view(B, K1, -1), z.view(B, K1, -1)
        return (a[:, 0].contiguous(), z[:, 0].contiguous(), a[:, 1:].contiguous(), z[:, 1:].contiguous(), q_emb)

    def _hip_vqa_forward(self, image_features, q_emb, want_a_orig):
        """ncx_vqa_forward / ncx_mlb_forward on the frozen weights of this module (packed once per device)."""
        B, K1 = image_features.size(0), self.knn_size + 1
        mw = self.__dict__.get("_mutan_weights")
        if mw is None or mw.t["wv"].device != image_features.device:
            mw = ops.vqa_weights(self.vqa_model)
            self.__dict__["_mutan_weights"] = mw
        feats = image_features.reshape(B * K1, -1).float().contiguous()
        idx = torch.arange(B * K1, device=feats.device, dtype=torch.int32).view(B, K1)
        return ops.vqa_forward(feats, idx, q_emb.float().contiguous(), mw, want_a_orig=want_a_orig)

    def refresh_vqa_weights(self):
        """Call after loading a VQA checkpoint: the stacked MUTAN weights of the HIP path are cached (and the packed weights of
        the HIP question encoder, which would also notice the change on their own)."""
        self.__dict__.pop("_mutan_weights", None)
        enc = getattr(self.vqa_model, "seq2vec", None)
        if hasattr(enc, "drop_hip_weights"):
            enc.drop_hip_weights()

    def forward(self, image_features, question_wids, answer_aids):
        raise NotImplementedError


def blackbox_scores(a_knns, answer_aids):
    """-softmax(a_knns)[b, k, answer_aids[b]]: the VQA model's own probability of the original answer on each
    candidate, sign-flipped because the likeliest images are the worst counterexamples (cx.py:122-136)."""
    aid = answer_aids.long().view(-1, 1, 1).expand(-1, a_knns.size(1), 1)
    return -(a_knns.gather(2, aid).squeeze(2) - torch.logsumexp(a_knns, dim=2)).exp()


class BlackBox(CXModelBase):
    """Scores candidates with the frozen VQA model alone (reference cx.py:114-136; README row 'Hard negative mining')."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.vqa_model.eval()

    def forward(self, image_features, question_wids, answer_aids):
        _, _, a_knns, _, _ = self.vqa_forward(image_features, question_wids)
        return blackbox_scores(a_knns, answer_aids)


class SemanticBaseline(CXModelBase):
    """Scores candidates by how far the VQA model's answer distribution moves away from the original answer, in an answer
    embedding space (reference cx.py:159-210; README row 'Semantic Baseline'):
        p = softmax(a_knns[b, k]);  s_k = lam (emb_pairs[aid] . p - p[aid]) - (1 - lam) log(p[aid] + 1e-8);  softmax_k(s)
    with emb_pairs the cosine Gram of the answer embedding.  The Gram is built on the device (ops.cosine_gram, once per
    embedding and device) and the scorer is one HIP launch per batch (ops.semantic_scores); a_knns come from the HIP MUTAN
    path.  There is no CPU fallback: on a CPU device `forward` raises.

    Kept from the reference: the constructor, `set_lambda`, `set_answer_embedding` (numpy array or tensor), `lam` (0.5 by
    default), the mutable `knn_size`, a `softmax` helper, the readable `emb_pairs` ([2000, 2000] zeros before an embedding is
    set), forward returning fp32 [B, K] probabilities with requires_grad=True (nothing trains), and state_dict keys
    (`vqa_model.*` only).  Deliberate differences (supersets):
      * both softmaxes subtract the max: equal wherever the reference is finite, finite for logits above ~88.7 (NaN there);
      * before set_answer_embedding the Gram is zeros of the logits' width (the reference's is [2000, 2000] whatever A is);
      * an answer id outside [0, A) raises IndexError (numpy wraps a negative one in the reference);
      * `emb_pairs` is a host copy of the device Gram, computed on first access (the reference computes it eagerly) and
        cached outside the module's state; the constructor does not print the VQA options.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dim_z = fusion_out_dim(self.vqa_model.opt["fusion"])
        self.emb = None
        self.lam = 0.5                     # cx.py:171 (default)
        self.__dict__["_grams"] = {}       # device -> device Gram of self.emb (not module state: checkpoints stay vqa_model.*)

    def set_lambda(self, lam):
        self.lam = lam

    def set_answer_embedding(self, emb):
        if isinstance(emb, torch.Tensor):
            emb = emb.detach()
        else:
            emb = np.asarray(emb)
        if emb.ndim != 2:
            raise ValueError("answer embedding must be [A, da], got %s" % (tuple(emb.shape),))
        self.emb = emb
        self.__dict__["_grams"] = {}

    @staticmethod
    def softmax(w):
        e = np.exp(np.asarray(w) - np.max(w))
        return e / np.sum(e)

    def _gram(self, device, A):
        grams = self.__dict__["_grams"]
        g = grams.get((device, A))
        if g is None:
            if self.emb is None:
                g = torch.zeros(A, A, dtype=torch.float32, device=device)
            else:
                if self.emb.shape[0] != A:
                    raise ValueError("answer embedding has %d rows, the VQA model scores %d answers" % (self.emb.shape[0], A))
                g = ops.cosine_gram(torch.as_tensor(self.emb).to(device=device, dtype=torch.float32))
            grams[(device, A)] = g
        return g

    @property
    def emb_pairs(self):
        if self.emb is None:
            return np.zeros((2000, 2000), np.float32)             # cx.py:168
        if not torch.cuda.is_available():
            raise ops._lib.NcxError("SemanticBaseline.emb_pairs is computed on the GPU (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
        return self._gram(dev, self.emb.shape[0]).cpu().numpy()

    def forward(self, image_features, question_wids, answer_aids):
        if not image_features.is_cuda:
            raise ops._lib.NcxError("SemanticBaseline runs on the GPU: move the inputs and the model there (no CPU fallback)")
        assert image_features.size(1) == self.knn_size + 1
        if self._hip_vqa_ok(image_features):
            with torch.no_grad():
                self.vqa_model.eval()
                q_emb = self.vqa_model.seq2vec(question_wids)
                _, _, a_knns, _ = self._hip_vqa_forward(image_features, q_emb, want_a_orig=False)
        else:
            _, _, a_knns, _, _ = self.vqa_forward(image_features, question_wids)
        a_knns = a_knns.float().contiguous()
        flag = torch.zeros(1, dtype=torch.int32, device=a_knns.device)
        scores = ops.semantic_scores(a_knns, answer_aids.to(a_knns.device), self._gram(a_knns.device, a_knns.size(2)),
                                     float(self.lam), bad_flag=flag)
        ops.check_semantic_ids(flag)            # (the reference reads its scores back to the host per batch as well)
        return scores.requires_grad_(True)      # cx.py:209


class SimilarityModel(CXModelBase):
    """Scores candidates by similarity to the original in image-feature and fusion space plus the VQA model's loss on the
    original answer (reference cx.py:490-518; no parameters of its own):
        scores[b, k] = cos(v_orig[b], v_knn[b, k]) + cos(z_orig[b], z_knn[b, k]) + cross_entropy(a_knns[b, k], answer_aids[b])
    The whole scorer is one HIP launch per batch (ops.similarity_scores: the reference loops over the candidates in Python,
    three torch ops each); z and a come from the HIP MUTAN path where it applies.  There is no CPU fallback: on a CPU device
    `forward` raises.

    Kept from the reference: the constructor, `dim_z`, the mutable `knn_size`, forward returning fp32 [B, knn_size] on the
    inputs' device without requires_grad (cx.py:518), the cosine rule of F.cosine_similarity (each norm clamped at 1e-8: an
    all-zero row scores 0), and state_dict keys (`vqa_model.*` only).  Deliberate differences (supersets):
      * knn_size may be 1..64 (CXModelBase's assert ties it to the width of image_features, as in the reference);
      * `trainable_vqa=True` is rejected (the reference detaches z and a here anyway: nothing would train);
      * an answer id outside [0, A) raises IndexError (F.cross_entropy's target check aborts or raises, by device, in the
        reference).
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.trainable_vqa:
            raise NotImplementedError("trainable_vqa=True is not supported by the HIP path (frozen VQA model only)")
        self.dim_z = fusion_out_dim(self.vqa_model.opt["fusion"])

    def forward(self, image_features, question_wids, answer_aids):
        if not image_features.is_cuda:
            raise ops._lib.NcxError("SimilarityModel runs on the GPU: move the inputs and the model there (no CPU fallback)")
        assert image_features.size(1) == self.knn_size + 1
        B, K1 = image_features.size(0), self.knn_size + 1
        _, z_orig, a_knns, z_knns, _ = self.vqa_forward(image_features, question_wids)
        dev = image_features.device
        feats = image_features.reshape(B * K1, -1).float().contiguous()       # the gathered block as the table, ids = arange
        idx = torch.arange(B * K1, device=dev, dtype=torch.int32).view(B, K1)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        scores = ops.similarity_scores(feats, idx, z_orig, z_knns, a_knns, answer_aids.to(dev), bad_flag=flag)
        ops.check_similarity_ids(flag)
        return scores                            # cx.py:518 (a fresh tensor: no requires_grad)


class PairwiseModel(CXModelBase):
    """The reference's pairwise scorer (cx.py:336-376; `counterexamples.py --pairwise`, knn_size = 2) is outside the accelerated
    path: the name exists so that the reference's import line (counterexamples.py:30-32) resolves against this package, and
    constructing it says so."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("PairwiseModel (--pairwise, knn_size = 2) is outside the accelerated path: it has no HIP "
                                  "implementation; use the reference's vqa.models.cx for it")


class NeuralModel(CXModelBase):
    def __init__(self, model_spec, dim_h, n_layers, emb, drop_p, **kwargs):
        super().__init__(vqa_model=kwargs["vqa_model"], knn_size=kwargs["knn_size"],
                         trainable_vqa=kwargs.get("trainable_vqa", False))
        if self.trainable_vqa:
            raise NotImplementedError("trainable_vqa=True is not supported by the HIP path (frozen VQA model only)")
        if not 3 <= self.knn_size <= 64:         # (the reference asserts knn_size == 24, cx.py:226; the kernels' 16-byte
            raise ValueError("knn_size must be in 3..64")     #  row windows need K + 1 >= 4 columns in the dist | rank block)
        if n_layers not in (1, 2, 3):
            raise ValueError("n_layers must be 1, 2 or 3")
        self.model_spec = dict(model_spec)
        fus = self.vqa_model.opt["fusion"]
        self.dim_v, self.dim_q, self.dim_z = fus["dim_v"], fus["dim_q"], fusion_out_dim(fus)
        self.ans_size = len(self.vqa_model.vocab_answers)
        self.dim_a = DIM_A
        self.dim_h, self.n_layers, self.drop_p = dim_h, n_layers, drop_p
        self._built_knn = self.knn_size

        self.answer_embedding = nn.Embedding(self.ans_size, self.dim_a)
        if emb is not None:
            assert emb.shape[1] == self.dim_a
            self.answer_embedding.weight.data = torch.as_tensor(emb, dtype=torch.float32)
        input_size = self.dim_v * 3 + self.dim_a * 2 + self.dim_z * 2 + self.dim_q + self.knn_size + 1
        self.linear_1 = nn.Linear(input_size, dim_h)
        if n_layers >= 2:
            self.linear_2 = nn.Linear(dim_h, dim_h)
        if n_layers >= 3:
            self.linear_3 = nn.Linear(dim_h, dim_h)
        self.out = nn.Linear(dim_h, 1)
        self.relu = nn.ReLU()
        self.drop = nn.Dropout(p=drop_p)
        self._pool = ops.WorkspacePool()
        self._step = 0
        self.dropout_seed = 42
        self.strict_ids = bool(kwargs.get("strict_ids", False))     # True: bad answer ids raise at the offending forward (host sync)

    # ---- the HIP hot path ---------------------------------------------------------------------------------
    def _param_fields(self):
        p = {"answer_embedding": self.answer_embedding.weight, "w1": self.linear_1.weight, "b1": self.linear_1.bias,
             "w_out": self.out.weight, "b_out": self.out.bias}
        if self.n_layers >= 2:
            p["w2"], p["b2"] = self.linear_2.weight, self.linear_2.bias
        if self.n_layers >= 3:
            p["w3"], p["b3"] = self.linear_3.weight, self.linear_3.bias
        return p

    def score_batch(self, batch: "ops.Batch"):
        """scores[B, K] for a device-resident ops.Batch (feature table + row indices: the gather of
        counterexamples.py:540-541 happens inside the kernels)."""
        if batch.img_idx.shape[1] != self._built_knn + 1:
            raise ValueError("linear_1 was built for knn_size=%d" % self._built_knn)
        fields = self._param_fields()
        names = tuple(fields)
        tensors = [fields[n] for n in names]
        for t in tensors:
            if not t.is_cuda:
                raise ops._lib.NcxError("NeuralModel parameters must live on the GPU: call .cuda() (no CPU fallback)")
        self._step += 1
        d = ops.make_dims(batch, H=self.dim_h, L=self.n_layers, da=self.dim_a, A=self.ans_size,
                          flags=ops.flags_from_spec(self.model_spec), training=self.training,
                          drop_p=self.drop_p if self.training else 0.0, seed=(self.dropout_seed << 32) ^ self._step)
        record = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
        call = dict(dims=d, batch=batch, names=names, pool=self._pool, record=record)      # per-call snapshot (re-entrant: see ops.WorkspacePool)
        return ops.NeuralCXFunction.apply(call, *tensors)

    _aid_host, _aid_event, _aid_pending, _aid_flag = None, None, False, None

    def check_answer_ids(self, wait=True):
        """Raises IndexError if the previous forward saw an answer id outside [0, ans_size) (what nn.Embedding raises at
        cx.py:280).  wait=False: only if the flag's copy has already landed (never blocks the host)."""
        if not self._aid_pending:
            return
        if self._aid_event is not None:
            if not wait and not self._aid_event.query():
                return
            self._aid_event.synchronize()
        self._aid_pending = False
        if bool(self._aid_host[0]):
            self._aid_flag.zero_()                                  # (sticky on the device until reported)
            raise IndexError("answer_aids outside [0, %d) in a previous forward" % self.ans_size)

    # The deferred verdict is collected wherever the caller synchronises anyway: a mode switch (the reference calls
    # cx_model.eval() / .train() around eval_model and at every epoch, counterexamples.py:320,451) and state_dict() (checkpoint
    # save, counterexamples.py:555) -- so a bad id in the last forward of an epoch or of an evaluation pass cannot be scored
    # silently and then checkpointed.
    def train(self, mode=True):
        self.check_answer_ids(wait=True)
        return super().train(mode)

    def state_dict(self, *args, **kwargs):
        self.check_answer_ids(wait=True)
        return super().state_dict(*args, **kwargs)

    def forward(self, image_features, question_wids, answer_aids):
        spec = self.model_spec
        B = image_features.size(0)
        assert image_features.size(1) == self.knn_size + 1                     # cx.py:263
        K, dev = self.knn_size, image_features.device
        if not spec.get("v_emb", True):                                         # cx.py:265-266
            image_features = torch.rand(B, K + 1, self.dim_v, device=dev)
        if spec.get("q_emb", True) or spec.get("z_emb", True):                  # cx.py:270-271
            a_orig, z_orig, a_knns, z_knns, q_emb = self.vqa_forward(image_features, question_wids)
        elif spec.get("a_emb", True):
            raise ValueError("model_spec with q_emb=z_emb=False needs a_emb=False (a_knns would be undefined)")
        if not spec.get("q_emb", True):                                         # cx.py:272-277
            q_emb = torch.rand(B, self.dim_q, device=dev)
        if not spec.get("z_emb", True):
            z_orig = torch.rand(B, self.dim_z, device=dev)
            z_knns = torch.rand(B, K, self.dim_z, device=dev)
        extra = {}
        if not spec.get("a_emb", True):                                         # cx.py:283-285
            a_knns = torch.rand(B, K, self.dim_a, device=dev)
            extra["a_emb_gt"] = torch.rand(B, self.dim_a, device=dev)
        if not spec.get("v_rank", True):                                        # cx.py:306-307
            extra["v_rank"] = torch.rand(B, K, K, device=dev)
        if spec.get("a_emb", True) and answer_aids.numel():
            # nn.Embedding raises on a bad index (cx.py:280); the kernels gather / scatter embedding rows by it.  No host
            # sync per forward: the ids are clamped for the kernels, the verdict goes to a device flag whose copy to pinned
            # host memory is read at the NEXT forward (long complete by then) or by check_answer_ids() -- the error of
            # step n surfaces as soon as its copy has landed (checked at every later forward) or when the caller asks.  The flag is
            # STICKY on the device (or-ed across forwards, cleared only when reported): the host runs ahead of the GPU, so the
            # copy of step n has usually not landed when step n + 1 is enqueued, and a later copy must still carry step n's verdict.
            self.check_answer_ids(wait=False)
            bad = ((answer_aids < 0) | (answer_aids >= self.ans_size)).any().view(1)
            if (self.strict_ids or dev.type != "cuda") and bool(bad):      # immediate raise, before anything is launched
                raise IndexError("answer_aids outside [0, %d)" % self.ans_size)
            answer_aids = answer_aids.clamp(0, self.ans_size - 1)
            if self._aid_host is None or self._aid_flag is None or self._aid_flag.device != dev:
                self._aid_host = torch.zeros(1, dtype=torch.bool).pin_memory() if dev.type == "cuda" else torch.zeros(1, dtype=torch.bool)
                self._aid_flag = torch.zeros(1, dtype=torch.bool, device=dev)
            self._aid_flag |= bad
            self._aid_host.copy_(self._aid_flag, non_blocking=True)
            if dev.type == "cuda":
                self._aid_event = torch.cuda.Event()
                self._aid_event.record(torch.cuda.current_stream(dev))
            self._aid_pending = True
        batch = ops.Batch.from_dense(image_features.float(), q_emb.float(), z_orig.float(), z_knns.float(),
                                     a_knns.float(), answer_aids, **extra)
        return self.score_batch(batch)


class _ScorerFunction(torch.autograd.Function):
    """scores = scorer(inputs; params) with the hand-written HIP backward (ncx_pairlin_backward / ncx_linctx_backward).
    `call` = {kind, dims, batch, names}: backward reads the dims, inputs and workspace of ITS forward from ctx."""

    @staticmethod
    def forward(ctx, call, *param_tensors):
        d, batch, names = call["dims"], call["batch"], call["names"]
        params = dict(zip(names, param_tensors))
        dev = batch.z_knns.device
        if call["kind"] == "pairlin":
            ws = ops.pairlin_workspace(d, dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            scores = ops.pairlin_forward(d, batch, params, ws, bad_flag=flag)
            ops.check_semantic_ids(flag)            # nn.Embedding / the feature indexing raise on a bad index (cx.py:408-414)
        else:
            ws = ops.linctx_workspace(d, dev)
            scores = ops.linctx_forward(d, batch.z_knns, params["w"], params["b"], ws)
        ctx.call, ctx.ws = call, ws
        ctx.save_for_backward(*param_tensors)
        return scores

    @staticmethod
    def backward(ctx, dscores):
        if ctx.ws is None:
            raise RuntimeError("backward ran twice on one forward (retain_graph is not supported)")
        call = ctx.call
        d, batch, names = call["dims"], call["batch"], call["names"]
        params = dict(zip(names, ctx.saved_tensors))
        grads = {n: torch.empty_like(t) for n, t in params.items()}
        dscores = dscores.float().contiguous()
        if call["kind"] == "pairlin":
            ops.pairlin_backward(d, batch, params, ctx.ws, dscores, grads)
        else:
            ops.linctx_backward(d, batch.z_knns, dscores, ctx.ws, grads["w"], grads["b"])
        ctx.ws = None
        return (None,) + tuple(grads[n] for n in names)


class _TrainableScorer(CXModelBase):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.trainable_vqa:
            raise NotImplementedError("trainable_vqa=True is not supported by the HIP path (frozen VQA model only)")

    def _score(self, call, fields):
        names = tuple(fields)
        for t in fields.values():
            if not t.is_cuda:
                raise ops._lib.NcxError("%s runs on the GPU: call .cuda() (no CPU fallback)" % type(self).__name__)
        call["names"] = names
        return _ScorerFunction.apply(call, *[fields[n] for n in names])


class LinearContext(_TrainableScorer):
    """cx.py:139-156: scores = linear(z_knns.view(B, K dz)), linear = nn.Linear(K dz, K).  Forward and backward run in the
    HIP library (ncx_linctx_forward / _backward); state_dict keys linear.weight, linear.bias (+ vqa_model.*)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dim_z = fusion_out_dim(self.vqa_model.opt["fusion"])
        self.linear = nn.Linear(self.knn_size * self.dim_z, self.knn_size)

    def forward(self, image_features, question_wids, answer_aids):
        if not image_features.is_cuda:
            raise ops._lib.NcxError("LinearContext runs on the GPU: move the inputs and the model there (no CPU fallback)")
        _, _, _, z_knns, _ = self.vqa_forward(image_features, question_wids)
        z_knns = z_knns.float().contiguous()
        batch = ops.Batch(None, None, None, None, z_knns, None)
        return self._score(dict(kind="linctx", dims=ops.linctx_dims(z_knns), batch=batch),
                           {"w": self.linear.weight, "b": self.linear.bias})


class PairwiseLinearModel(_TrainableScorer):
    """cx.py:379-425: per candidate, relu(out(relu(linear(cat(v_orig, v_other, q_emb, z_orig, z_other, a_emb))))).  The concat is
    never built (ncx_pairlin_forward / _backward, csrc/ncx_scorers.hip); state_dict keys answer_embedding.weight, linear.*,
    out.* (+ vqa_model.*).  An answer id outside [0, A) raises IndexError (one host sync per forward)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert self.knn_size == 24                              # cx.py:384
        fus = self.vqa_model.opt["fusion"]
        self.dim_v, self.dim_q, self.dim_z = fus["dim_v"], fus["dim_q"], fusion_out_dim(fus)
        self.dim_h = ops.PAIRLIN_H
        self.dim_a = ops.PAIRLIN_H
        self.answer_embedding = nn.Embedding(len(self.vqa_model.vocab_answers), self.dim_a)
        self.linear = nn.Linear((2 * self.dim_v) + self.dim_q + (2 * self.dim_z) + self.dim_a, self.dim_h)
        self.out = nn.Linear(self.dim_h, 1)
        self.relu = nn.ReLU()

    def forward(self, image_features, question_wids, answer_aids):
        if not image_features.is_cuda:
            raise ops._lib.NcxError("PairwiseLinearModel runs on the GPU: move the inputs and the model there (no CPU fallback)")
        assert image_features.size(1) - 1 == self.knn_size     # cx.py:403
        _, z_orig, _, z_knns, q_emb = self.vqa_forward(image_features, question_wids)
        batch = ops.Batch.from_dense(image_features.float(), q_emb.float(), z_orig.float(), z_knns.float(),
                                     z_knns.float(), answer_aids)
        fields = {"answer_embedding": self.answer_embedding.weight, "w": self.linear.weight, "b": self.linear.bias,
                  "w_out": self.out.weight, "b_out": self.out.bias}
        return self._score(dict(kind="pairlin", dims=ops.pairlin_dims(batch, self.answer_embedding.num_embeddings), batch=batch),
                           fields)


class _ContrastiveFunction(torch.autograd.Function):
    """h = relu(linear(cat(v, z))) for the P images of every example, with the hand-written HIP backward
    (ncx_contrastive_forward / _backward).  `call` = {dims, batch}: backward reads the dims, inputs and workspace of ITS forward."""

    @staticmethod
    def forward(ctx, call, w, b):
        d, batch = call["dims"], call["batch"]
        dev = batch.z_knns.device
        ws = ops.contrastive_workspace(d, dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        h = ops.contrastive_forward(d, batch, w, b, ws, bad_flag=flag)
        ctx.call, ctx.ws = call, ws
        return h

    @staticmethod
    def backward(ctx, dh):
        if ctx.ws is None:
            raise RuntimeError("backward ran twice on one forward (retain_graph is not supported)")
        d, batch = ctx.call["dims"], ctx.call["batch"]
        gw = torch.empty(ops.CONTRASTIVE_H, d.dv + d.dz, dtype=torch.float32, device=dh.device)
        gb = torch.empty(ops.CONTRASTIVE_H, dtype=torch.float32, device=dh.device)
        ops.contrastive_backward(d, batch, ctx.ws, gw, gb, dh=dh.float().contiguous())
        ctx.ws = None
        return None, gw, gb


class ContrastiveModel(CXModelBase):
    """cx.py:428-487: a siamese embedding of the knn_size + 1 images of an example, h = relu(linear(cat(v_i, z_i))) [B, P, 300],
    trained by contrastive.py with ContrastiveLoss on distances.  Forward and backward run in the HIP library
    (csrc/ncx_contrastive.hip) through an autograd.Function, so the reference's own loss and torch.optim.Adam train it unchanged.
    State keys answer_embedding.weight (constructed, never used, never given a gradient: cx.py:440-441, 458), linear.weight
    [300, dim_v + dim_mm] (columns v | z), linear.bias (+ vqa_model.*).  knn_size is mutable (the reference flips it 2 <-> 24
    around evaluation, contrastive.py:270, 287); 1..64 here."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.trainable_vqa:
            raise NotImplementedError("trainable_vqa=True is not supported by the HIP path (frozen VQA model only)")
        fus = self.vqa_model.opt["fusion"]
        self.dim_v, self.dim_q, self.dim_z = fus["dim_v"], fus["dim_q"], fusion_out_dim(fus)
        self.dim_h = ops.CONTRASTIVE_H
        self.dim_a = ops.CONTRASTIVE_H
        self.answer_embedding = nn.Embedding(len(self.vqa_model.vocab_answers), self.dim_a)
        self.linear = nn.Linear(self.dim_v + self.dim_z, self.dim_h)
        self.relu = nn.ReLU()

    def _embed(self, feats, img_idx, z_orig, z_knns):
        if not (feats.is_cuda and self.linear.weight.is_cuda):
            raise ops._lib.NcxError("ContrastiveModel runs on the GPU: move the inputs and the model there (no CPU fallback)")
        batch = ops.Batch(feats.float().contiguous(), img_idx, None, z_orig.float().contiguous(), z_knns.float().contiguous(), None)
        d = ops.contrastive_dims(batch)
        return _ContrastiveFunction.apply(dict(dims=d, batch=batch), self.linear.weight, self.linear.bias)

    def forward(self, image_features, question_wids, answer_aids):
        B, P = image_features.size(0), image_features.size(1)
        assert P == self.knn_size + 1                              # cx.py:451
        _, z_orig, _, z_knns, _ = self.vqa_forward(image_features, question_wids)
        feats = image_features.reshape(B * P, -1)
        idx = torch.arange(B * P, device=feats.device, dtype=torch.int32).view(B, P)
        return self._embed(feats, idx, z_orig, z_knns)

    def get_hidden(self, v, z):
        """relu(linear(cat(v, z))) for one image per row (cx.py:470-472): the library embeds at least two images per example, so
        every row is presented twice and slot 0 returned."""
        B = v.size(0)
        idx = torch.arange(B, device=v.device, dtype=torch.int32).view(B, 1).expand(B, 2).contiguous()
        return self._embed(v, idx, z, z.reshape(B, 1, -1))[:, 0]

    @torch.no_grad()
    def get_scores(self, h_orig, h_knns):
        """Distances [B, P - 1] of every neighbour's embedding to the original's (cx.py:478-487), a device tensor."""
        h = torch.cat([h_orig.unsqueeze(1), h_knns], dim=1).float().contiguous()
        d = ops._lib.NcxContrastiveDims()
        d.B, d.P, d.dv, d.dz, d.n_img = h.size(0), h.size(1), self.dim_v, self.dim_z, 1
        return ops.contrastive_distances(d, h=h)
