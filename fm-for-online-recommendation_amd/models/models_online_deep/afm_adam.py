"""AFMAdam: the attentional factorization machine (Xiao et al. 2017) on the gfx950 kernels (fmx_afm_forward / fmx_afm_step;
pairwise-ranking training on the same logit: fmx_afm_pair_*, fit_pairs / run_pair_experiment with attention=True; listwise
training: fmx_afm_list_*, fit_lists / run_list_experiment with attention=True).

The model (include/fmx.h, DESIGN.md section 3 "AFM"): per sample, with e_f = x_f V[row_f] and w_f the first-order weight, over
the P = F (F - 1) / 2 pairs in the order i = 0..F-2, j = i+1..F-1,

    q_ij = e_i * e_j,   s_ij = H . relu(W q_ij + b),   a_ij = softmax over the sample's pairs of s_ij,
    logit = bias + sum_f w_f x_f + P . sum_ij a_ij q_ij

with W, b = attention_linear.weight / .bias, H and P the reference's parameters (reference afm_adam.py:39-41).

Where this class departs from the reference's code, which cannot run as written (SURVEY.md row afm_adam.py):
  * the reference builds its "interaction layer" from per-field squares (afm_adam.py:62), so its shapes only line up at F = 3;
    here the interaction layer is the pairwise products of the paper;
  * the reference defines `activation = F.relu` (:63) and never applies it; here the ReLU of the paper is applied;
  * `.view` with a float (:67, :69), `loss.data[0]` and the undefined self.verbose / evaluate / eval_metric (:120-123, :167)
    are gone: fit() returns the per-epoch mean log-loss of the training (and validation) data and reports no other metric;
  * the reference's fit() uses ONE persistent torch.optim.Adam over every parameter (:93).  The default update_rule 'adam' is
    that optimizer's SparseAdam form on the tables -- a row's moments move only when the row occurs in the batch (a dense Adam
    would keep moving every row on its old moments) -- and one persistent torch.optim.Adam on the attention parameters.
Parameters are created in the reference's RNG order (:25-41), so one torch seed gives the reference's initial model.
There is no CPU path: constructing the class without a ROCm GPU raises.
"""
from time import time

import numpy as np
import torch
import torch.nn as nn

import fmx
from fmx.afm import AFMEngine, AfmOpt

from ._base import OnlineFMBase, _FieldView
from ._ranking import RankingTraining


class AFMAdam(RankingTraining, nn.Module):
    _name = "AFMAdam"
    _logit_family = "afm"       # RankingTraining refuses the pure FM's pair and list methods and its mining by name

    def __init__(self, feature_sizes, embedding_size=4, attention_size=4, n_epochs=64, batch_size=256, num_classes=1, b=0.99,
                 n=0.003, use_cuda=True, update_rule="adam", ftrl=None, adam=None, adagrad=None, fused_optimizer=False):
        """update_rule: 'adam' (default: SparseAdam on the tables, a persistent Adam on the attention parameters), 'adagrad',
        'signadam' (a fresh Adam per step), 'sgd' or 'ftrl' (settings ftrl=dict(alpha, beta, l1, l2)) -- the tables' rules of
        the other classes; the attention parameters take what the hidden layers of DeepFM / NFM take under the same rule.
        Every rule's learning rate is n.
        fused_optimizer: False keeps the attention parameters on torch (a torch optimizer under 'adam' / 'adagrad', element-wise
        ops under the others) after every fmx_afm_step.  True, for every update_rule: their rule is applied inside the step's
        gradient reduction (fmx_afm_step_opt: update_embedding is one call and no torch op touches the parameters), and fit()
        uploads the data once and runs each epoch's full batches as one fmx_afm_stream call.  The two settings agree to rounding,
        not bit for bit (the kernels' 1-ulp reciprocal and square root against torch's)."""
        super().__init__()
        if not (use_cuda and torch.cuda.is_available()):
            raise RuntimeError(f"{self._name}: this build runs the hot path in gfx950 kernels only -- it needs use_cuda=True "
                               "and a ROCm GPU (there is no CPU or PyTorch fallback; use the reference for CPU runs)")
        if update_rule not in ("signadam", "sgd", "ftrl", "adagrad", "adam"):
            raise ValueError(update_rule)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.field_size = len(feature_sizes)
        self.feature_sizes = feature_sizes
        self.embedding_size = embedding_size
        self.attention_size = attention_size
        self.n_epochs = n_epochs
        self.batch_size = batch_size
        self.num_classes = num_classes
        self.use_cuda = use_cuda
        self.update_rule = update_rule
        self.fused_optimizer = bool(fused_optimizer)
        k, t = embedding_size, attention_size

        # ---- the reference's RNG order (afm_adam.py:30-41) ----
        bias0 = torch.tensor(b)
        self.n = torch.nn.Parameter(torch.tensor(n), requires_grad=False)
        first = [nn.Embedding(fs, 1).weight.data for fs in feature_sizes]
        second = [nn.Embedding(fs, k).weight.data for fs in feature_sizes]
        lin = nn.Linear(k, t)
        H0 = torch.randn(t)
        P0 = torch.randn(k)
        self._bias_shape = tuple(bias0.shape)

        self._ftrl = dict(alpha=0.05, beta=1.0, l1=0.0, l2=0.0)
        if ftrl:
            self._ftrl.update(ftrl)
        self._adam = dict(beta1=0.9, beta2=0.999, eps=1e-8)
        if adam:
            self._adam.update({k_: float(v) for k_, v in adam.items() if k_ in self._adam})
        self._adagrad = dict(eps=1e-10)
        if adagrad:
            self._adagrad.update({k_: float(v) for k_, v in adagrad.items() if k_ in self._adagrad})
        adaptive = update_rule in ("adagrad", "adam")
        layout = "ftrl" if update_rule == "ftrl" else "moments" if adaptive else "weights"
        self._table = fmx.FlatTable(feature_sizes, k, layout=layout, device=self.device, ftrl=self._ftrl)
        self._load_weights(first, second, bias0)
        del first, second
        self._hyper = self._make_hyper(n)

        # one flat device buffer [W | b | H | P] behind the attention parameters: the kernels read it, the modules see views of it
        self._attn_flat = torch.cat([lin.weight.detach().reshape(-1), lin.bias.detach(), H0, P0]).float().to(self.device).contiguous()
        self.attention_linear = lin.to(self.device)
        self.H = nn.Parameter(torch.empty(0, device=self.device))
        self.P = nn.Parameter(torch.empty(0, device=self.device))
        o = 0
        for prm, shape in ((self.attention_linear.weight, (t, k)), (self.attention_linear.bias, (t,)), (self.H, (t,)), (self.P, (k,))):
            m = int(np.prod(shape))
            prm.data = self._attn_flat[o:o + m].view(shape)
            o += m
        self._attn_opt = None
        self._attn_fused = None     # fused_optimizer=True: the flat moments and the step count instead (fmx.AfmOpt)
        if self.fused_optimizer:    # the policy of _apply_attention: ftrl tables go with signadam on the attention parameters
            arule = "signadam" if update_rule == "ftrl" else update_rule
            b1, b2 = self._betas()
            self._attn_fused = AfmOpt(self._attn_flat.numel(), arule, lr=float(n), beta1=b1, beta2=b2, device=self.device,
                                      eps=self._adam["eps"] if arule == "adam" else self._adagrad["eps"] if arule == "adagrad" else 1e-8)
        elif adaptive:     # the model's ONE persistent optimizer over the attention parameters (the tables keep their moments)
            params = self._attn_params()
            if update_rule == "adam":
                self._attn_opt = torch.optim.Adam(params, lr=float(n), betas=self._betas(), eps=self._adam["eps"])
            else:
                self._attn_opt = torch.optim.Adagrad(params, lr=float(n), eps=self._adagrad["eps"])
        self._engine = AFMEngine(self._table, self._attn_flat, t, max_batch=max(int(batch_size), 64))
        self.first_order_embeddings = [_FieldView(self._table, f, False) for f in range(self.field_size)]
        self.second_order_embeddings = [_FieldView(self._table, f, True) for f in range(self.field_size)]

    def _attn_params(self):
        return [self.attention_linear.weight, self.attention_linear.bias, self.H, self.P]

    # what is honestly shared with the other classes: the hyper-parameters, the table <-> reference weights, the input path,
    # the index check and the FTRL state
    _betas = OnlineFMBase._betas
    _make_hyper = OnlineFMBase._make_hyper
    _load_weights = OnlineFMBase._load_weights
    _export_weights = OnlineFMBase._export_weights
    bias = OnlineFMBase.bias
    _inputs = OnlineFMBase._inputs
    _inputs_fast = OnlineFMBase._inputs_fast
    strict_index_check = True
    check_index_flag = OnlineFMBase.check_index_flag
    _after_step = OnlineFMBase._after_step
    ftrl_state_dict = OnlineFMBase.ftrl_state_dict
    load_ftrl_state_dict = OnlineFMBase.load_ftrl_state_dict

    # ------------------------------------------------------------------------------------------------------
    # forward / predict (reference afm_adam.py:43-74, 170-191)
    # ------------------------------------------------------------------------------------------------------
    def forward(self, Xi, Xv):
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        B = self._engine.forward(self._hyper, idx_d, xv_d)
        self._after_step()
        return self._engine.logit[:B].clone()

    def predict_proba(self, Xi, Xv):
        self.eval()
        return torch.sigmoid(self.forward(Xi, Xv)).cpu().numpy()

    def predict(self, Xi, Xv):
        return self.predict_proba(Xi, Xv) > 0.5

    def _scoring(self, item_fields, candidates, full):
        """RankingTraining's hook for recommend / rank: the attentional scorer (whatever `full`), after this class's check that
        the one item field of candidates=None is a field."""
        fields = self._item_fields(item_fields)
        if candidates is None and len(fields) == 1 and not 0 <= fields[0] < self.field_size:
            raise ValueError(f"item field {fields[0]}: not a field of 0..{self.field_size - 1}")
        item_fields, cand_idx, cand_xv = self._candidate_rows(item_fields, candidates)
        rec, afm = fmx.recommend, (self._attn_flat, self.attention_size)
        return (rec.AFMScorer(afm, self._table.k),
                rec.AFMCandidates(self._table, afm, item_fields, cand_idx, cand_xv, hyper=self._hyper))

    # ------------------------------------------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------------------------------------------
    def _apply_attention(self, g):
        """The attention parameters' update under the model's rule -- the policy OnlineFMBase._fit applies to the hidden layers:
        sgd the plain step; signadam and ftrl the closed form of a fresh Adam's first step; adam / adagrad the persistent
        optimizer."""
        lr = float(self.n)
        with torch.no_grad():
            if self._attn_opt is not None:
                o = 0
                for prm in self._attn_params():
                    prm.grad = g[o:o + prm.numel()].view(prm.shape).clone()
                    o += prm.numel()
                self._attn_opt.step()
            elif self.update_rule == "sgd":
                self._attn_flat.sub_(g, alpha=lr)
            else:
                self._attn_flat.sub_(lr * g / (g.abs() + 1e-8))

    def _fit_step(self, engine_step, *args, **kwargs):
        """One step of the whole model through engine_step (AFMEngine.step / pair_step / list_step) under the model's rule; with
        fused_optimizer=False the attention parameters' rule follows on torch.  Returns the step's mean loss."""
        engine_step(self._hyper, self.update_rule, *args, opt=self._attn_fused, **kwargs)
        if self._attn_fused is None:
            self._apply_attention(self._engine.grad)
        out = self._engine.loss_out[0].clone()
        self._after_step()
        return out

    def update_embedding(self, Xi, Xv, Y):
        """One mini-batch step of the whole model (tables and attention) on BCE-with-logits; returns the mean loss."""
        self.train()
        idx_d, xv_d, y_d = self._inputs(Xi, Xv, Y)
        if y_d.numel() != idx_d.shape[0]:
            raise ValueError(f"Target size ({y_d.numel()}) must be the same as input size ({idx_d.shape[0]})")
        return self._fit_step(self._engine.step, idx_d, xv_d, y_d)

    # ---- pairwise-ranking (BPR) training on the attentional logit (fmx_afm_pair_*; the pair objective of the other classes) ----
    def _pair_refusal(self, method, attention, loss="pair"):
        """The default keeps the other classes' reading of these methods -- the pair or list loss of the pure FM logit, which this
        model does not have; attention=True trains on the logit forward() gives."""
        if not attention:
            self._pure_fm_only(method, loss, own=("attention", "the attentional FM's"))

    def fit_pairs(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None, attention=False):
        """OnlineFMBase.fit_pairs's arguments; attention=True: one mini-batch pair step of the whole model (tables and attention)
        on -log(sigmoid(z_pos - z_neg) + margin) over the logit forward() gives, inv_b = 1 / pairs; returns the mean pair loss.
        fused_optimizer=True: one fmx_afm_pair_step_opt call; False: fmx_afm_pair_step, then the attention parameters' rule on
        torch, as update_embedding splits."""
        self._refuse_hard_negatives("fit_pairs", negatives)
        self._pair_refusal("fit_pairs", attention)
        self.train()
        rows, xv = self._pair_rows(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)
        return self._fit_step(self._engine.pair_step, rows, xv, margin=margin)

    # ---- listwise (sampled-softmax) training on the attentional logit (fmx_afm_list_*; the list objective of FMAdam) ----
    def _list_entry(self, method, negatives, n_neg, attention):
        """What fit_lists / run_list_experiment decide before they look at the model: without attention the pure FM's refusal,
        first; then the limit of negatives, then the mined negatives' refusal, then the corrected list loss's (a
        PopularityNegatives with correct=True: this model's list kernels have no log-Q correction)."""
        self._pair_refusal(method, attention, "list")
        if negatives is None or fmx.pairwise.hard_negatives(negatives) is not None or fmx.pairwise.popularity_negatives(negatives) is not None:
            self._list_limit(method, n_neg)
        self._refuse_hard_negatives(method, negatives)
        self._refuse_corrected_lists(method, negatives)

    def fit_lists(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, attention=False):
        """FMAdam.fit_lists's arguments; attention=True: one mini-batch list step of the whole model (tables and attention) on
        -log softmax of the positive's logit among its list's, over the logit forward() gives, inv_b = 1 / lists; returns the
        mean list loss.  At most 15 negatives per positive; the bias does not move.  fused_optimizer=True: one
        fmx_afm_list_step_opt call; False: fmx_afm_list_step, then the attention parameters' rule on torch, as fit_pairs splits."""
        self._list_entry("fit_lists", negatives, n_neg, attention)
        self.train()
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        rows, xv, G = self._list_rows("fit_lists", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
        return self._fit_step(self._engine.list_step, rows, G, xv)

    def _unit_experiment(self, start, n, rows_of, online_run, right, fit_unit):
        """run_pair_experiment / run_list_experiment behind their refusals, for n units (pairs, lists): rows_of() -> the assembled
        (rows, xv, G), G rows per unit.  fused_optimizer=True: one upload and ONE call online_run(rows, xv, G, logits) for the n G
        logits before each unit's update; False: the host loop of fit_unit(rows, xv, G, i), a one-unit step whose own forward
        leaves the unit's logits in the engine.  right(z [m, G]) -> [m] bool: the unit was predicted correctly."""
        if n == 0:
            return self._experiment_result(start, None)
        rows, xv, G = rows_of()
        if self._attn_fused is not None:
            logits = torch.empty(n * G, dtype=torch.float32, device=self.device)
            online_run(rows, xv, G, logits)
            return self._experiment_result(start, right(logits.view(n, G)).to(torch.uint8))
        return self._experiment_result(start, self._host_stream_loop(n, lambda i: fit_unit(rows, xv, G, i),
                                                                     lambda: right(self._engine.logit[:G].view(1, G))[0]))

    def run_list_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, attention=False):
        """FMAdam.run_list_experiment's arguments and 4-tuple; attention=True: for every list predict the positive's rank among
        its negatives from the logits before the list's update (correct: rank 0, no negative's logit >= the positive's), then
        fit on that list alone.  fused_optimizer=True: one upload and ONE fmx_afm_list_online_run call; False: the host loop of
        one-list fit_lists(attention=True) -- the same protocol."""
        self._list_entry("run_list_experiment", negatives, n_neg, attention)
        start = time()
        self.train()
        idx_d, xv_d, _ = self._inputs(Xi, Xv)

        def fit_one(rows, xv, G, i):
            fields, lst = self._item_fields(item_fields), rows[G * i:G * (i + 1)]
            self.fit_lists(lst[:1], None if xv is None else xv[G * i:G * i + 1], fields,
                           negatives=lst[1:, fields].reshape(1, G - 1, -1), attention=True)
        return self._unit_experiment(
            start, idx_d.shape[0],
            lambda: self._list_rows("run_list_experiment", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator),
            lambda rows, xv, G, logits: self._engine.list_online_run(self._hyper, self.update_rule, rows, G, xv, self._attn_fused,
                                                                     logits=logits),
            lambda z: (z[:, 1:] >= z[:, :1]).sum(1) == 0, fit_one)

    # (mine_negatives: RankingTraining's, which refuses it for this model by name)

    def run_pair_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None,
                            attention=False):
        """OnlineFMBase.run_pair_experiment's arguments and 4-tuple; attention=True: for every pair predict z_pos > z_neg from the
        logits before the pair's update, then fit on that pair alone.  fused_optimizer=True: one upload and ONE
        fmx_afm_pair_online_run call; False: the host loop of one-pair fit_pairs(attention=True) -- the same protocol."""
        self._refuse_hard_negatives("run_pair_experiment", negatives)
        self._pair_refusal("run_pair_experiment", attention)
        start = time()
        self.train()
        rows, xv = self._pair_rows(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)

        def fit_one(rows, xv, G, i):
            fields = self._item_fields(item_fields)
            pos, pos_xv, neg = self._pair_at(rows, xv, fields, i)
            self.fit_pairs(pos, pos_xv, fields, negatives=neg, margin=margin, attention=True)
        return self._unit_experiment(
            start, rows.shape[0] // 2, lambda: (rows, xv, 2),
            lambda rows, xv, G, logits: self._engine.pair_online_run(self._hyper, self.update_rule, rows, xv, self._attn_fused,
                                                                     margin=margin, logits=logits),
            lambda z: z[:, 0] > z[:, 1], fit_one)

    def _mean_logloss(self, Xi, Xv, y, chunk=16384):
        """The mean BCE-with-logits over a data set, evaluated by batches (reference eval_by_batch, :143-165)."""
        total, N = 0.0, len(y)
        self.eval()
        for o in range(0, N, chunk):
            idx_d, xv_d, y_d = self._inputs(Xi[o:o + chunk], Xv[o:o + chunk], y[o:o + chunk])
            B = self._engine.forward(self._hyper, idx_d, xv_d, y_d, loss="logits")
            total += float(self._engine.loss_b[:B].double().sum())
            self._after_step()
        return total / N

    def fit(self, Xi_train, Xv_train, y_train, Xi_valid=None, Xv_valid=None, y_valid=None):
        """The reference's epoch x batch loop (afm_adam.py:76-141).  -> (train_result, valid_result): per epoch the mean
        log-loss of the training data and of the validation data (empty without it)."""
        F = self.field_size
        Xi_train = np.asarray(Xi_train).reshape((-1, F))
        Xv_train = np.asarray(Xv_train, dtype=np.float32).reshape((-1, F))
        y_train = np.asarray(y_train, dtype=np.float32).reshape(-1)
        is_valid = Xi_valid is not None and len(Xi_valid) > 0
        if is_valid:
            Xi_valid = np.asarray(Xi_valid).reshape((-1, F))
            Xv_valid = np.asarray(Xv_valid, dtype=np.float32).reshape((-1, F))
            y_valid = np.asarray(y_valid, dtype=np.float32).reshape(-1)
        x_size = Xi_train.shape[0]
        train_result, valid_result = [], []
        if self._attn_fused is not None:      # the training data on the device once: the epochs' batches are slices of it
            idx_d, xv_d, y_d = self._inputs(Xi_train, Xv_train, y_train)
        for epoch in range(self.n_epochs):
            epoch_begin_time = time()
            if self._attn_fused is not None:
                self._fit_epoch_fused(idx_d, xv_d, y_d)
            else:
                for offset in range(0, x_size, self.batch_size):
                    end = min(x_size, offset + self.batch_size)
                    self.update_embedding(Xi_train[offset:end], Xv_train[offset:end], y_train[offset:end])
            train_loss = self._mean_logloss(Xi_train, Xv_train, y_train)
            train_result.append(train_loss)
            print("[%d] loss: %.6f time: %.1f s" % (epoch + 1, train_loss, time() - epoch_begin_time))
            if is_valid:
                valid_loss = self._mean_logloss(Xi_valid, Xv_valid, y_valid)
                valid_result.append(valid_loss)
                print("[%d] valid loss: %.6f time: %.1f s" % (epoch + 1, valid_loss, time() - epoch_begin_time))
        return train_result, valid_result

    def _fit_epoch_fused(self, idx_d, xv_d, y_d):
        """One epoch over device-resident data in the order of fit()'s batch loop: the full batches as ONE fmx_afm_stream call,
        a ragged last batch as one fmx_afm_step_opt call with inv_b = 1 / its size -- the bits of update_embedding batch by
        batch.  The index flag is read once per call, not per step."""
        self.train()
        e, B = self._engine, int(self.batch_size)
        n_full = idx_d.shape[0] // B
        cut = n_full * B
        if n_full:
            e.stream(self._hyper, self.update_rule, idx_d[:cut], None if xv_d is None else xv_d[:cut], y_d[:cut], B, n_full,
                     self._attn_fused)
            if self.strict_index_check:
                self.check_index_flag()
        if cut < idx_d.shape[0]:
            e.step(self._hyper, self.update_rule, idx_d[cut:], None if xv_d is None else xv_d[cut:], y_d[cut:], opt=self._attn_fused)
            if self.strict_index_check:
                self.check_index_flag()

    def run_experiment(self, data_Xi, data_Xv, data_Y):
        """predict() over the data, then the confusion matrix and its checkpoints every 1,000 samples (afm_adam.py:193-223)."""
        pred = np.asarray(self.predict(data_Xi, data_Xv)).reshape(-1)
        start = time()
        y = np.asarray(data_Y).reshape(-1)
        return self._report(y, pred == y, start)

    @staticmethod
    def _report(y, hit, start):
        """(seconds, accuracy %, last roc point, confusion matrix) of the predictions `hit` marks as right against the labels y,
        with the checkpoints of the other classes' run_experiment: every 1,000 samples and at the last sample."""
        n = len(y)
        pos = y == 1
        tp, fn = np.cumsum(pos & hit), np.cumsum(pos & ~hit)
        tn, fp = np.cumsum(~pos & hit), np.cumsum(~pos & ~hit)
        accuracy, roc = [], []
        for i in sorted(set(range(0, n, 1000)) | {n - 1}):
            roc.append({"tpr": tp[i] / (tp[i] + fn[i] + 1e-16), "fpr": fp[i] / (fp[i] + tn[i] + 1e-16)})
            accuracy.append((tp[i] + tn[i]) / (i + 1) * 100)
        cm = {"tp": int(tp[-1]), "fp": int(fp[-1]), "tn": int(tn[-1]), "fn": int(fn[-1])}
        return time() - start, float(accuracy[-1]), {k: float(v) for k, v in roc[-1].items()}, cm

    def run_online_experiment(self, data_Xi, data_Xv, data_Y):
        """The online protocol of the other classes' run_experiment (reference fm_adam.py:90-119), which the reference's AFM
        lacks: predict a sample (sigmoid(logit) > 0.5), then fit on it, one sample at a time -> (seconds, accuracy %,
        {'tpr', 'fpr'}, {'tp', 'fp', 'tn', 'fn'}).  run_experiment keeps the reference's predict-only behaviour.
        fused_optimizer=True: one upload and ONE fmx_afm_online_run call -- the bits of a loop of predict() and
        update_embedding() over one-sample batches; the index flag is read once.  fused_optimizer=False: that loop itself."""
        F = self.field_size
        Xi = np.asarray(data_Xi).reshape((-1, F))
        Xv = np.asarray(data_Xv, dtype=np.float32).reshape((-1, F))
        Y = np.asarray(data_Y, dtype=np.float32).reshape(-1)
        N = len(Y)
        if N == 0:
            raise ValueError("run_online_experiment: no samples")
        start = time()
        if self._attn_fused is not None:
            self.train()
            idx_d, xv_d, y_d = self._inputs(Xi, Xv, Y)
            logits = torch.empty(N, dtype=torch.float32, device=self.device)
            self._engine.online_run(self._hyper, self.update_rule, idx_d, xv_d, y_d, self._attn_fused, logits=logits)
            pred = (torch.sigmoid(logits) > 0.5).cpu().numpy()
            if self.strict_index_check:
                self.check_index_flag()
        else:
            pred = np.zeros(N, dtype=bool)
            for i in range(N):
                pred[i] = bool(np.asarray(self.predict(Xi[i:i + 1], Xv[i:i + 1])).reshape(-1)[0])
                self.update_embedding(Xi[i:i + 1], Xv[i:i + 1], Y[i:i + 1])
        return self._report(Y, pred == (Y == 1), start)     # the predictions taken before each sample's update

    # ------------------------------------------------------------------------------------------------------
    # state (the reference's keys) and pickling
    # ------------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        first, second, bias = self._export_weights()
        sd = {"bias": bias.reshape(self._bias_shape).clone(), "n": self.n.detach().clone(),
              "H": self.H.detach().cpu().clone(), "P": self.P.detach().cpu().clone()}
        for i in range(self.field_size):
            sd[f"first_order_embeddings.{i}.weight"] = first[i]
        for i in range(self.field_size):
            sd[f"second_order_embeddings.{i}.weight"] = second[i]
        sd["attention_linear.weight"] = self.attention_linear.weight.detach().cpu().clone()
        sd["attention_linear.bias"] = self.attention_linear.bias.detach().cpu().clone()
        return sd

    def load_state_dict(self, state_dict, strict=True):
        sd = {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v) for k, v in state_dict.items()}
        want = set(self.state_dict().keys())
        if strict and set(sd.keys()) != want:
            raise RuntimeError(f"state_dict keys differ: missing {sorted(want - set(sd))}, unexpected {sorted(set(sd) - want)}")
        first = [sd[f"first_order_embeddings.{i}.weight"].float().cpu() for i in range(self.field_size)]
        second = [sd[f"second_order_embeddings.{i}.weight"].float().cpu() for i in range(self.field_size)]
        self._load_weights(first, second, sd["bias"].float().cpu())
        with torch.no_grad():
            self.n.copy_(sd["n"].float().cpu())
            self._hyper = self._make_hyper(float(self.n))
            for prm, key in zip(self._attn_params(), ("attention_linear.weight", "attention_linear.bias", "H", "P")):
                prm.copy_(sd[key].float().to(self.device))
            if self._attn_opt is not None:
                for g in self._attn_opt.param_groups:
                    g["lr"] = float(self.n)
            if self._attn_fused is not None:
                self._attn_fused.c.lr = float(self.n)

    def optimizer_state_dict(self):
        """{'table': FlatTable.export_moments_state(), 'attention': the attention optimizer's state_dict} on the CPU for the
        rules with moments ('adam', 'adagrad'); None for the others.  With fused_optimizer=True, under every rule: 'attention' is
        {'m', 'v', 'step'} -- the flat moments in the layout [W | b | H | P] and the attention parameters' step count -- and
        'table' is None unless the rule keeps moments."""
        if self._attn_fused is not None:
            return {"table": self._table.export_moments_state() if self._table.layout == "moments" else None,
                    "attention": self._attn_fused.state_dict()}
        if self._attn_opt is None:
            return None
        st = self._attn_opt.state_dict()
        st = {"state": {i: {k_: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k_, v in s.items()}
                        for i, s in st["state"].items()}, "param_groups": st["param_groups"]}
        return {"table": self._table.export_moments_state(), "attention": st}

    def load_optimizer_state_dict(self, st):
        if self._attn_fused is not None:
            if st.get("table") is not None:
                self._table.load_moments_state(st["table"])
                self._table.step = int(st["table"]["step"])
            self._attn_fused.load_state_dict(st["attention"])
            return
        if self._attn_opt is None:
            raise ValueError("load_optimizer_state_dict: this model does not use update_rule 'adam' or 'adagrad'")
        self._table.load_moments_state(st["table"])
        self._table.step = int(st["table"]["step"])
        self._attn_opt.load_state_dict(st["attention"])

    def __getstate__(self):
        return {"ctor": dict(feature_sizes=list(self.feature_sizes), embedding_size=self.embedding_size,
                             attention_size=self.attention_size, n_epochs=self.n_epochs, batch_size=self.batch_size,
                             num_classes=self.num_classes, update_rule=self.update_rule, ftrl=dict(self._ftrl),
                             adam=dict(self._adam), adagrad=dict(self._adagrad), fused_optimizer=self.fused_optimizer),
                "state_dict": {k: v.cpu() for k, v in self.state_dict().items()},
                "ftrl_state": self.ftrl_state_dict(), "optimizer_state": self.optimizer_state_dict()}

    def __setstate__(self, state):
        c = state["ctor"]
        AFMAdam.__init__(self, c["feature_sizes"], embedding_size=c["embedding_size"], attention_size=c["attention_size"],
                         n_epochs=c["n_epochs"], batch_size=c["batch_size"], num_classes=c["num_classes"],
                         update_rule=c["update_rule"], ftrl=c["ftrl"], adam=c["adam"], adagrad=c["adagrad"],
                         fused_optimizer=c.get("fused_optimizer", False))
        self.load_state_dict(state["state_dict"])
        if state.get("ftrl_state") is not None:
            self.load_ftrl_state_dict(state["ftrl_state"])
        if state.get("optimizer_state") is not None:
            self.load_optimizer_state_dict(state["optimizer_state"])

    def __str__(self):
        return (f"{self._name}-Feature_Sizes{self.feature_sizes}-Embedding_Sizes{self.embedding_size}-"
                f"Attention_Size{self.attention_size}-Num_Classes{self.num_classes}")
