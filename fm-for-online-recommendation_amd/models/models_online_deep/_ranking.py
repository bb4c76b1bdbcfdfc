"""Ranking training of the model classes, defined once: pairs (BPR: fmx_fm_pair_*), lists (sampled softmax: fmx_fm_list_*, and
its log-Q corrected form fmx_fm_list_*_q), in-batch negatives (fmx_fm_inbatch_*), mined negatives (fmx_fm_mine_negatives) and
popularity-sampled ones (fmx_alias_sample_negatives).

RankingTraining is a mixin of OnlineFMBase (FMAdam, the DeepFM / NFM classes) and of AFMAdam.  It holds the pure FM's public
methods, and what the three families share under them: the rows of positives and negatives, the host predict-then-fit loop, the
experiments' 4-tuple and the refusals by name.  The host class brings _name, device, field_size, feature_sizes, update_rule,
_engine, _hyper, _table, _inputs, _after_step and train(); the pure FM also _device_loop_ok.
NetworkPairTraining is the pair objective on the whole network's logit (DeepFMAdam / NFMAdam); AFMAdam's own, on the attentional
logit, is in afm_adam.py.
"""
from time import time

import numpy as np
import torch

import fmx


def _scoring_of(model, item_fields, candidates, full):
    """recommend's and rank's first step: the refusal of the classes with an MLP without full=True, then the class's hook"""
    if getattr(model, "_has_mlp", False) and not full:
        raise NotImplementedError(f"{model._name}.recommend: the MLP on the bi-interaction vector does not decompose over "
                                  "the context / item field split; recommend(..., full=True) scores every pair through "
                                  "the network")
    return model._scoring(item_fields, candidates, full)


class RankingTraining:
    # whose logit the class trains: "fm" (the pure FM: FMAdam), "mlp" (the classes with an MLP) or "afm"
    _logit_family = "fm"

    @staticmethod
    def _item_fields(item_fields):
        """One field index or a sequence of them -> a list of ints"""
        return [int(f) for f in (item_fields if hasattr(item_fields, "__len__") else [item_fields])]

    # ---- recommendation and ranking evaluation (fmx/recommend.py) ----
    def _candidate_rows(self, item_fields, candidates):
        """recommend's and rank's candidates: (item fields, cand_idx, cand_xv) -- every row of the one item field when
        candidates is None, else the caller's (cand_Xi, cand_Xv)."""
        item_fields = self._item_fields(item_fields)
        F = self.field_size
        if candidates is None:
            if len(item_fields) != 1:
                raise ValueError("candidates=None needs exactly one item field (its rows are the candidates)")
            f = item_fields[0]
            cand_idx = torch.zeros((self.feature_sizes[f], F), dtype=torch.int32, device=self.device)
            cand_idx[:, f] = torch.arange(self.feature_sizes[f], dtype=torch.int32, device=self.device)
            cand_xv = None
        else:
            cand_idx, cand_xv = candidates
        return item_fields, cand_idx, cand_xv

    def _scoring(self, item_fields, candidates, full):
        """The class's hook: -> (its fmx.recommend scorer, its candidates object over _candidate_rows(item_fields, candidates))"""
        raise NotImplementedError

    def recommend(self, Xi, Xv, item_fields, K, candidates=None, exclude=None, full=False):
        """Top-K candidates for every context row (fmx/recommend.py; fmx_fm_topk, fmx_mlp_topk, fmx_afm_topk).  Xi / Xv: [U, F]
        full-width rows whose item columns are ignored (Xv may be None: all ones).  candidates=None: every row of the one item
        field, a position is that field's local index; else (cand_Xi [N, F], cand_Xv or None) whose non-item columns are
        ignored.  exclude: per-user position lists or a CSR pair (offsets, positions).  Returns numpy (positions int64 [U, K], -1
        padded; logits fp32 [U, K], -inf padded), each row by logit descending, then position ascending.
        full=True scores every pair through the whole network (fmx_mlp_topk): for DeepFMAdam / NFMAdam the logit forward()
        returns, for DeepFMOnn / NFMOnn the logit whose sigmoid forward() returns; on FMAdam it is the default call, and AFMAdam
        accepts it for the signature: its score is always the whole model's, the exact logit forward() gives the combined sample."""
        scorer, cands = _scoring_of(self, item_fields, candidates, full)
        pos, logit = fmx.recommend.scorer_topk(scorer, self._table, Xi, Xv, cands, K, exclude=exclude, hyper=self._hyper)
        return pos.cpu().numpy(), logit.cpu().numpy()

    def rank(self, Xi, Xv, item_fields, targets, candidates=None, exclude=None, full=False, filtered=False):
        """The rank of held-out target positions among all candidates for every context row (fmx/recommend.py; fmx_fm_rank,
        fmx_mlp_rank, fmx_afm_rank): the number of eligible candidates recommend's order puts in front of the target, i.e. its
        0-based index in an unbounded recommend row.  Xi / Xv, item_fields, candidates, exclude, full: as recommend.  targets: [U],
        [U, T] or U lists of positions in the sense of recommend's results (-1: padding).  filtered: the user's other targets are
        not counted.  Returns numpy (ranks int64 [U, T], -1: not eligible; scores fp32 [U, T], -inf there; n_cand int64 [U])."""
        scorer, cands = _scoring_of(self, item_fields, candidates, full)
        out = fmx.recommend.scorer_rank(scorer, self._table, Xi, Xv, cands, targets, exclude=exclude, hyper=self._hyper,
                                        filtered=filtered)
        return tuple(o.cpu().numpy() for o in out)

    def evaluate_ranking(self, Xi, Xv, item_fields, targets, candidates=None, exclude=None, full=False, filtered=False,
                         ks=(1, 5, 10)):
        """fmx.recommend.ranking_metrics (hr@K, ndcg@K, mrr, auc, n) of rank(...)."""
        ranks, _, n_cand = self.rank(Xi, Xv, item_fields, targets, candidates, exclude, full, filtered)
        return fmx.recommend.ranking_metrics(torch.from_numpy(ranks), torch.from_numpy(n_cand), ks=ks)

    # ---- the refusals, by class and method name ----
    def _refuse_hard_negatives(self, method, negatives):
        """The classes and modes fmx_fm_mine_negatives does not score for: negatives='hard' there is refused by name."""
        if fmx.pairwise.hard_negatives(negatives) is not None:
            raise NotImplementedError(f"{self._name}.{method}: negatives='hard' mines under the pure FM score (FMAdam; "
                                      "fmx_fm_mine_negatives); mining under the whole network's score or the attentional score "
                                      "needs the scan of fmx_mlp_topk / fmx_afm_topk fed by draws")

    def _pure_fm_only(self, method, loss="pair", own=None):
        """Refuse `method` (the pair or the list loss of fmx_fm_pair_* / fmx_fm_list_*) on a class whose logit is not the pure
        FM's.  own: (keyword, "whose logit") of the class's own form of the method, which the refusal then points to."""
        family = self._logit_family
        if family == "fm":
            return
        parts = [f"{self._name}.{method}: the {loss} loss is built for the pure FM logit (FMAdam)"]
        epilogue = "pair" if loss == "pair" else "softmax"
        if family == "mlp":
            parts.append(f"the classes with an MLP would need the {epilogue} epilogue inside the MLP section")
        elif own is None:
            parts.append(f"the attentional FM would need the {epilogue} epilogue behind its own forward")
        if own is not None:
            parts.append(f"{method}(..., {own[0]}=True) trains on the {loss} loss of {own[1]} logit")
        raise NotImplementedError("; ".join(parts))

    # ---- positives and their negatives as rows ----
    def _pair_rows(self, Xi, Xv, item_fields, negatives, n_neg, candidates, generator):
        """-> (rows int32 [2P, F], xv [2P, F] or None) on the device: P = B * n_neg pairs, row 2p the positive, 2p + 1 the negative"""
        return self._negative_rows(fmx.pairwise.assemble_pairs, Xi, Xv, item_fields, negatives, n_neg, candidates, generator)

    def _negative_rows(self, assemble, Xi, Xv, item_fields, negatives, n_neg, candidates, generator):
        """The positives with their negatives -- given, mined ("hard" / a HardNegatives), drawn by popularity (a
        PopularityNegatives) or drawn uniformly (None) -- laid out by `assemble` (fmx.pairwise.assemble_pairs / assemble_lists)"""
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        fields = self._item_fields(item_fields)
        hard = fmx.pairwise.hard_negatives(negatives)
        if hard is not None:
            negatives, _ = self.mine_negatives(idx_d, xv_d, fields, hard.n_draw, n_neg=n_neg, candidates=candidates,
                                               exclude=hard.exclude, generator=generator, refresh_every=hard.refresh_every)
        popular = fmx.pairwise.popularity_negatives(negatives)
        if popular is not None:
            negatives, _ = self._sample_popular(idx_d, fields, popular, n_neg, candidates, generator)
        if negatives is None:
            src = candidates if candidates is not None else [self.feature_sizes[f] for f in fields]
            negatives = fmx.pairwise.sample_negatives(idx_d, fields, src, n_neg=n_neg, generator=generator)
        self._fast_inputs_pending = True      # the negatives' indices are range-checked by the kernels
        return assemble(idx_d, xv_d, fields, negatives)

    @staticmethod
    def _pair_at(rows, xv, fields, i):
        """Pair i of assembled pair rows as a one-pair fit takes it: (the positive's row, its values, the negative's item columns)"""
        return rows[2 * i:2 * i + 1], None if xv is None else xv[2 * i:2 * i + 1], rows[2 * i + 1:2 * i + 2, fields]

    # ---- the online experiments' host side ----
    def _host_stream_loop(self, n, fit_one, read_pred):
        """The predict-then-fit loop on the host: for i < n, fit_one(i) -- one step on element i alone -- then read_pred(), the
        element's prediction from the step's own forward, the logits before its update -> uint8 [n] on the device.  One index
        check after the loop (the experiment's), no sync inside it."""
        out = torch.empty(n, dtype=torch.uint8, device=self.device)
        strict, self.strict_index_check = self.strict_index_check, False
        try:
            for i in range(n):
                fit_one(i)
                out[i] = read_pred()
        finally:
            self.strict_index_check = strict
        return out

    def _experiment_result(self, start, pred):
        """The 4-tuple of run_pair_experiment / run_list_experiment from the per-element hits [n] on the device (None or empty:
        no element, nothing was launched); reads the index flag once"""
        if pred is None or len(pred) == 0:
            return time() - start, 0.0, [], {"correct": 0, "wrong": 0}
        self._engine.check_error_flag()
        self._fast_inputs_pending = False
        hit = pred.cpu().numpy().astype(bool)
        n = len(hit)
        correct = np.cumsum(hit)
        accuracy = [float(correct[i] / (i + 1) * 100) for i in sorted(set(range(0, n, 1000)) | {n - 1})]
        counts = {"correct": int(correct[-1]), "wrong": int(n - correct[-1])}
        return time() - start, accuracy[-1], accuracy, counts

    def _walk_mined_blocks(self, Xi, Xv, hard, walk):
        """The block loop of the online experiments under mined negatives (pairs and lists): the positives in blocks of
        hard.remine_every (None: one block), walk(idx, xv, block) on each with `block` the HardNegatives that mines it under the
        model the blocks before it have trained (refresh_every = 1 per block) -- its exclusions cut to the block's rows -> the
        list of walk's results"""
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        B = idx_d.shape[0]
        step = B if hard.remine_every is None else hard.remine_every
        block = fmx.pairwise.HardNegatives(hard.n_draw, None, 1)
        excl = fmx.recommend.exclusions_csr(hard.exclude, B, "cpu")
        out = []
        for b0 in range(0, B, max(step, 1)):
            b1 = min(B, b0 + step)
            if excl[0] is not None:
                off, pos = excl
                block.exclude = (off[b0:b1 + 1] - off[b0], pos[int(off[b0]):int(off[b1])])
            out.append(walk(idx_d[b0:b1], None if xv_d is None else xv_d[b0:b1], block))
        return out

    @staticmethod
    def _cat(parts):
        parts = [p for p in parts if p is not None]
        return torch.cat(parts) if parts else None

    # ------------------------------------------------------------------------------------------------------
    # pairwise-ranking (BPR) training of the pure FM (fmx/pairwise.py, fmx_fm_pair_*): for a context, score the observed item
    # above a sampled one -- loss -log(sigmoid(z_pos - z_neg) + margin), margin 0 being BPR
    # ------------------------------------------------------------------------------------------------------
    def fit_pairs(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None):
        """One mini-batch pair step under the model's update rule; returns the loss tensor (the mean pair loss), as
        update_embedding does.  Xi / Xv: the positive samples [B, F] (Xv may be None: all ones).  negatives: the item columns of
        every positive's negatives, [B, n_neg, m] for m item fields ([B, m]: one each); None draws n_neg per positive uniformly
        (fmx.pairwise.sample_negatives) from `candidates` ([N, m] items) or, by default, from the item fields' vocabularies --
        never the row's own item, deterministic under a seeded `generator`.
        negatives="hard" (or a fmx.pairwise.HardNegatives carrying n_draw = 32, exclude, refresh_every = 1): every positive's
        n_neg negatives are mined by mine_negatives -- the best of n_draw drawn candidates under the current FM score.
        negatives=fmx.pairwise.PopularityNegatives(weights, ...): n_neg draws per positive in proportion to weights ** power
        (fmx_alias_sample_negatives); the pair loss has no log-Q correction, so its `correct` is ignored here."""
        if self._logit_family != "fm":
            self._refuse_hard_negatives("fit_pairs", negatives)
        self._pure_fm_only("fit_pairs")
        self.train()
        rows, xv = self._pair_rows(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)
        self._engine.pair_step(self._hyper, self.update_rule, rows, xv, margin=margin)
        out = self._engine.loss_out[0].clone()
        self._after_step()
        return out

    def run_pair_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None):
        """The online protocol restated for pairs: for every pair predict (z_pos > z_neg), then fit on that pair alone ->
        (seconds, pairwise accuracy in %, the accuracy at every pair i with i % 1000 == 0 and at the last, {"correct", "wrong"}).
        On the device (fmx_fm_pair_online_run: one wavefront walks the stream) where run_experiment's loop runs there; otherwise
        a loop over fit_pairs on one pair at a time -- the same bits.
        negatives="hard" (or a fmx.pairwise.HardNegatives): the stream is mined in blocks of remine_every positives (None: once,
        up front), the candidates refreshed before each block, and the loop above runs on the block."""
        if self._logit_family != "fm":
            self._refuse_hard_negatives("run_pair_experiment", negatives)
        self._pure_fm_only("run_pair_experiment")
        start = time()
        self.train()
        hard = fmx.pairwise.hard_negatives(negatives)

        def walk(idx, xv, negs):
            rows, xv = self._pair_rows(idx, xv, item_fields, negs, n_neg, candidates, generator)
            return self._pair_loop(rows, xv, item_fields, margin)
        preds = self._walk_mined_blocks(Xi, Xv, hard, walk) if hard is not None else [walk(Xi, Xv, negatives)]
        return self._experiment_result(start, self._cat(preds))

    def _pair_loop(self, rows, xv, item_fields, margin):
        """The predict-then-fit loop over assembled pair rows -> the per-pair predictions uint8 [n] on the device (None: no pair)"""
        n, e = rows.shape[0] // 2, self._engine
        if n == 0:
            return None
        if self._device_loop_ok():
            return e.pair_online_run(self._hyper, self.update_rule, rows, xv, margin=margin)[0]
        fields = self._item_fields(item_fields)

        def fit_one(i):
            pos, pos_xv, neg = self._pair_at(rows, xv, fields, i)
            self.fit_pairs(pos, pos_xv, fields, negatives=neg, margin=margin)
        return self._host_stream_loop(n, fit_one, lambda: e.logit[0] > e.logit[1])

    # ---- listwise (sampled-softmax) training of the pure FM (fmx_fm_list_*): softmax cross-entropy of the observed item against
    #      its n_neg negatives -- 1 + n_neg rows per positive where the pair form carries 2 n_neg, each negative weighted by its
    #      share of the probability mass ----
    def _list_limit(self, method, count, what="n_neg = {}"):
        limit = fmx._lib.LIST_MAX_G - 1
        if not 1 <= int(count) <= limit:
            raise ValueError(f"{self._name}.{method}: {what.format(count)}: a list holds 1 to {limit} negatives")

    def _list_rows(self, method, idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator):
        """-> (rows int32 [B G, F], xv or None, G) on the device: B lists of the positive and its G - 1 negatives"""
        rows, xv = self._negative_rows(fmx.pairwise.assemble_lists, idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
        G = rows.shape[0] // idx_d.shape[0]
        if G - 1 > fmx._lib.LIST_MAX_G - 1:
            self._list_limit(method, G - 1, "{} negatives per positive")
        return rows, xv, G

    def fit_lists(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None):
        """One mini-batch list step under the model's update rule; returns the loss tensor (the mean list loss), as fit_pairs
        does.  Every positive of Xi / Xv [B, F] and its negatives form one list; the loss is -log softmax of the positive's
        logit among the list's.  negatives: what fit_pairs takes -- the negatives' item columns [B, n_neg, m] ([B, m]: one each),
        None for n_neg uniform draws per positive, "hard" or a fmx.pairwise.HardNegatives for the n_neg best of n_draw drawn
        candidates under the current FM score (mine_negatives).  At most 15 negatives per positive.  The bias does not move.
        negatives=fmx.pairwise.PopularityNegatives(weights, ...): n_neg draws per positive in proportion to weights ** power
        (fmx_alias_sample_negatives); with its correct=True (the default) the step is fmx_fm_list_step_q -- log Q of every row's
        item, the positive's included, is subtracted from the row's logit in front of the softmax."""
        self._pure_fm_only("fit_lists", "list")
        popular = fmx.pairwise.popularity_negatives(negatives)
        if negatives is None or fmx.pairwise.hard_negatives(negatives) is not None or popular is not None:
            self._list_limit("fit_lists", n_neg)
        self.train()
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        corr = None
        if popular is not None and popular.correct:
            negatives, corr = self._sample_popular(idx_d, self._item_fields(item_fields), popular, n_neg, candidates, generator)
        rows, xv, G = self._list_rows("fit_lists", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
        if corr is None:
            self._engine.list_step(self._hyper, self.update_rule, rows, G, xv)
        else:
            self._engine.list_step_q(self._hyper, self.update_rule, rows, G, corr.reshape(-1), xv)
        out = self._engine.loss_out[0].clone()
        self._after_step()
        return out

    # ---- in-batch sampled softmax of the pure FM (fmx_fm_inbatch_*): the other rows' items are every row's negatives -- B - 1
    #      negatives per positive from the B rows the batch holds anyway, where fit_lists gathers 1 + n_neg rows per positive ----
    def fit_in_batch(self, Xi, Xv, item_fields, log_q=None, mask_duplicates=True, candidates=None):
        """One mini-batch in-batch step under the model's update rule; returns the loss tensor (the mean loss), as fit_lists
        does.  The positives Xi / Xv [B, F] alone: row i's loss is -log softmax of score(context i, item i) among
        score(context i, item j) over the batch's items j, the score recommend serves.  log_q: None; an array [B], log Q of every
        row's item, subtracted from that item's logits (Yi et al. 2019: in-batch negatives arrive in proportion to their
        popularity); or a fmx.pairwise.PopularityNegatives, whose log q is gathered at candidates.positions_of(items) --
        `candidates` (a fmx.recommend.Candidates over the same item fields) is then required, and an item that is no candidate
        or is never drawn takes the sampler's floor.  mask_duplicates: rows that hold the same item (fmx.pairwise.in_batch_keys)
        are left out of each other's softmax; False: every other row is a negative.  The bias does not move."""
        return self._fit_in_batch("fit_in_batch", Xi, Xv, item_fields, log_q, mask_duplicates, candidates, None)

    def fit_in_batch_bank(self, Xi, Xv, item_fields, log_q=None, mask_duplicates=True, candidates=None, bank=None):
        """fit_in_batch with a cross-batch item bank.  bank: a fmx.pairwise.ItemBank (fmx_fm_inbatch_bank_step): the items of
        earlier batches it keeps are further negatives of every row, and this batch's items are pushed into it behind the
        update; None is fit_in_batch, bit for bit.  The bank must agree with the other arguments: keyed exactly when
        mask_duplicates (the keys are then fmx.pairwise.item_keys', which hold across batches), corrected exactly when log_q is
        given; a mismatch is a ValueError that names the argument."""
        return self._fit_in_batch("fit_in_batch_bank", Xi, Xv, item_fields, log_q, mask_duplicates, candidates, bank)

    def _fit_in_batch(self, method, Xi, Xv, item_fields, log_q, mask_duplicates, candidates, bank):
        self._pure_fm_only(method, "list")
        self.train()
        if bank is not None:
            if not isinstance(bank, fmx.pairwise.ItemBank):
                raise ValueError(f"{self._name}.{method}: bank must be a fmx.pairwise.ItemBank or None, got {type(bank).__name__}")
            if bank.keyed != bool(mask_duplicates):
                raise ValueError(f"{self._name}.{method}: mask_duplicates={bool(mask_duplicates)} needs a bank with "
                                 f"keyed={bool(mask_duplicates)}; bank.keyed is {bank.keyed}")
            if bank.corrected != (log_q is not None):
                raise ValueError(f"{self._name}.{method}: log_q {'given' if log_q is not None else 'None'} needs a bank with "
                                 f"corrected={log_q is not None}; bank.corrected is {bank.corrected}")
            if bank.kp != self._table.kp:
                raise ValueError(f"{self._name}.{method}: bank.kp = {bank.kp}, the table's kp = {self._table.kp}")
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        fields = self._item_fields(item_fields)
        corr = self._in_batch_log_q(idx_d, fields, log_q, candidates)
        if bank is None:
            key = fmx.pairwise.in_batch_keys(idx_d, fields) if mask_duplicates else None
            self._engine.inbatch_step(self._hyper, self.update_rule, idx_d, fields, xv_d, corr=corr, key=key)
        else:
            key = fmx.pairwise.item_keys(idx_d, fields, np.diff(np.asarray(self._table.offsets_host))) if mask_duplicates else None
            self._engine.inbatch_bank_step(self._hyper, self.update_rule, idx_d, fields, bank, xv_d, corr=corr, key=key)
        out = self._engine.loss_out[0].clone()
        self._after_step()
        return out

    def _in_batch_log_q(self, idx_d, fields, log_q, candidates):
        """fit_in_batch's log_q -> fp32 [B] on the device, or None"""
        B = idx_d.shape[0]
        popular = fmx.pairwise.popularity_negatives(log_q)
        if popular is not None:
            if candidates is None:
                raise ValueError(f"{self._name}.fit_in_batch: log_q=PopularityNegatives(...) needs candidates (a "
                                 "fmx.recommend.Candidates): its log q is read at candidates.positions_of(items)")
            if popular.N != candidates.N:
                raise ValueError(f"{self._name}: PopularityNegatives holds {popular.N} weights for {candidates.N} candidate positions")
            logq = popular.table(self.device)[2]
            own = candidates.positions_of(idx_d[:, fields], fields).long()
            listed = own >= 0
            corr = torch.where(listed, logq[own.clamp(min=0)], torch.full((B,), float("-inf"), device=self.device))
            return corr.clamp(min=popular.floor_logq()).contiguous()
        if log_q is None:
            return None
        corr = torch.as_tensor(log_q).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if corr.numel() != B:
            raise ValueError(f"{self._name}.fit_in_batch: log_q holds {corr.numel()} values for {B} rows")
        return corr

    def run_list_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None):
        """The online protocol restated for lists: for every positive of Xi / Xv and its negatives predict the positive's rank
        among them, then fit on that list alone -> (seconds, top-1 accuracy in %, the accuracy at every list i with
        i % 1000 == 0 and at the last, {"correct", "wrong"}); correct: rank 0, no negative scores as high as the positive.
        negatives: what fit_lists takes; at most 15 per positive.  On the device (fmx_fm_list_online_run: one workgroup walks the
        stream) where run_experiment's loop runs there and the table has no sort split; otherwise a loop over fit_lists on one
        list at a time -- the same bits.  negatives="hard" (or a fmx.pairwise.HardNegatives): blocks of remine_every positives,
        as run_pair_experiment walks them.  negatives=fmx.pairwise.PopularityNegatives(...): the host loop of one-list fit_lists
        calls, each drawing its own negatives; the rank is read from the step's uncorrected logits (the serving score)."""
        self._pure_fm_only("run_list_experiment", "list")
        hard = fmx.pairwise.hard_negatives(negatives)
        popular = fmx.pairwise.popularity_negatives(negatives)
        if negatives is None or hard is not None or popular is not None:
            self._list_limit("run_list_experiment", n_neg)
        start = time()
        self.train()

        def walk(idx, xv, negs):
            return self._list_loop(idx, xv, item_fields, negs, n_neg, candidates, generator)
        if hard is not None:
            ranks = self._walk_mined_blocks(Xi, Xv, hard, walk)
        elif popular is not None:
            idx_d, xv_d, _ = self._inputs(Xi, Xv)
            ranks = [self._popular_list_loop(idx_d, xv_d, item_fields, popular, n_neg, candidates, generator)]
        else:
            idx_d, xv_d, _ = self._inputs(Xi, Xv)
            ranks = [walk(idx_d, xv_d, negatives)]
        ranks = self._cat(ranks)
        return self._experiment_result(start, None if ranks is None else ranks == 0)

    def _list_loop(self, idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator):
        """The predict-then-fit loop over the positives idx_d [n, F] and their negatives -> the positives' ranks uint8 [n] on the
        device (None: no list)"""
        n, e = idx_d.shape[0], self._engine
        if n == 0:
            return None
        rows, xv, G = self._list_rows("run_list_experiment", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
        if self._device_loop_ok() and e.list_online_run_fits(self.field_size, self._table.kp):
            return e.list_online_run(self._hyper, self.update_rule, rows, G, xv)[0]
        fields = self._item_fields(item_fields)

        def fit_one(i):
            lst = rows[G * i:G * (i + 1)]
            self.fit_lists(lst[:1], None if xv is None else xv[G * i:G * i + 1], fields, negatives=lst[1:, fields].reshape(1, G - 1, -1))
        return self._host_stream_loop(n, fit_one, lambda: (e.logit[1:G] >= e.logit[0]).sum())

    def _popular_list_loop(self, idx_d, xv_d, item_fields, popular, n_neg, candidates, generator):
        """The predict-then-fit loop under popularity-sampled negatives: one fit_lists call per positive, which draws that list's
        negatives (the sampler's exclusions cut to the row) -> the positives' ranks uint8 [n] on the device (None: no list)"""
        n, e, G = idx_d.shape[0], self._engine, 1 + int(n_neg)
        if n == 0:
            return None
        whole = popular.exclude
        off, pos = fmx.recommend.exclusions_csr(whole, n, "cpu")

        def fit_one(i):
            if off is not None:
                popular.exclude = (off[i:i + 2] - off[i], pos[int(off[i]):int(off[i + 1])])
            self.fit_lists(idx_d[i:i + 1], None if xv_d is None else xv_d[i:i + 1], item_fields, negatives=popular, n_neg=n_neg,
                           candidates=candidates, generator=generator)
        try:
            return self._host_stream_loop(n, fit_one, lambda: (e.logit[1:G] >= e.logit[0]).sum())
        finally:
            popular.exclude = whole

    def _refuse_corrected_lists(self, method, negatives):
        """The list steps outside the pure FM have no corrected form (fmx_fm_list_*_q is the pure FM's): a PopularityNegatives
        with correct=True is refused there by name"""
        popular = fmx.pairwise.popularity_negatives(negatives)
        if popular is not None and popular.correct and self._logit_family != "fm":
            raise NotImplementedError(f"{self._name}.{method}: the log-Q corrected list loss is built for the pure FM logit (FMAdam; "
                                      "fmx_fm_list_step_q); pass PopularityNegatives(..., correct=False) to train this class on "
                                      "popularity-sampled negatives without the correction")

    # ---- hard negatives (fmx.pairwise.mine_negatives, fmx_fm_mine_negatives) and the seeds of every device-side draw ----
    mining_seed = 0      # the Philox seed of mine_negatives and of the popularity sampler when no generator is given

    def _next_draw(self, generator):
        """(seed, offset) of the next mining or sampling call: generator.initial_seed() or mining_seed, and the model's count of
        such calls, which pickling carries"""
        seed = int(generator.initial_seed()) if generator is not None else int(self.mining_seed)
        offset = int(getattr(self, "_mining_offset", 0))
        self._mining_offset = offset + 1
        return seed, offset

    def _sample_popular(self, idx_d, fields, popular, n_neg, candidates, generator):
        """n_neg popularity-sampled negatives for every positive row of idx_d [B, F] (fmx_alias_sample_negatives under _next_draw's
        seed and offset): never the row's own item nor one of popular.exclude's positions -> (items int64 [B, n_neg, m] in the
        order of fields, what fit_pairs takes as negatives; log Q fp32 [B, 1 + n_neg] of every list row's item, the positive's
        first -- a positive the table never draws takes log(2^-24 / N)).  candidates: [N, m] items (None: every row of the one
        item field); popular's weights hold one entry per such position.  A row with fewer than n_neg eligible draws among its
        n_try raises ValueError (one host read per call, as in mine_negatives)."""
        pw, dev, B, m = fmx.pairwise, self.device, idx_d.shape[0], len(fields)
        items = idx_d[:, fields].long()
        if candidates is None:
            if m != 1:
                raise ValueError("candidates=None needs exactly one item field: the product of several fields' vocabularies "
                                 "cannot be enumerated -- pass the candidate items [N, m]")
            cand, N, own = None, int(self.feature_sizes[fields[0]]), items[:, 0]
        else:
            cand = torch.as_tensor(candidates).to(device=dev, dtype=torch.int64).reshape(-1, m)
            N, own = cand.shape[0], pw.candidate_positions(items, cand)
        if popular.N != N:
            raise ValueError(f"{self._name}: PopularityNegatives holds {popular.N} weights for {N} candidate positions")
        thresh, alias, logq = popular.table(dev)
        off, pos = fmx.recommend.exclusions_csr(popular.exclude, B, dev)
        seed, offset = self._next_draw(generator)
        n_try = popular.tries(n_neg)
        neg_pos, neg_logq = pw.alias_sample(thresh, alias, logq, n_neg, n_try, own.to(torch.int32).contiguous(), seed, offset, 0,
                                            off, pos)
        if bool((neg_pos < 0).any()):
            raise ValueError(f"{self._name}: a row has fewer than {int(n_neg)} eligible draws among its n_try = {n_try} (the others "
                             "were its own item or excluded): raise PopularityNegatives(n_try=...) up to 1024")
        at = neg_pos.long()
        neg_items = at.unsqueeze(-1) if cand is None else cand[at.reshape(-1)].reshape(B, int(n_neg), m)
        listed = (own >= 0) & (own < N)
        own_logq = torch.where(listed, logq[own.clamp(0, N - 1)], torch.full_like(neg_logq[:, 0], float("-inf")))
        corr = torch.cat([own_logq.clamp(min=popular.floor_logq())[:, None], neg_logq], dim=1).contiguous()
        return neg_items, corr

    def _mining_candidates(self, fields, candidates, refresh_every):
        """The fmx.recommend.Candidates of the last (item_fields, candidates), kept on the model and refreshed from the table
        every refresh_every mining calls.  They carry value 1 in the item columns."""
        kept = getattr(self, "_mining_kept", None)
        if kept is None or kept["fields"] != fields or kept["source"] is not candidates:
            rec = fmx.recommend
            if candidates is None:
                if len(fields) != 1:
                    raise ValueError("candidates=None needs exactly one item field: the product of several fields' vocabularies "
                                     "cannot be enumerated -- pass the candidate items [N, m]")
                cands = rec.Candidates.whole_field(self._table, fields[0], hyper=self._hyper)
            else:
                items = torch.as_tensor(candidates).to(device=self.device, dtype=torch.int32).reshape(-1, len(fields))
                cand_idx = torch.zeros((items.shape[0], self.field_size), dtype=torch.int32, device=self.device)
                cand_idx[:, fields] = items
                cands = rec.Candidates(self._table, fields, cand_idx, None, hyper=self._hyper)
            self._mining_kept = kept = {"fields": list(fields), "source": candidates, "cands": cands, "age": 0}
        elif kept["age"] >= int(refresh_every):
            kept["cands"].refresh()
            kept["age"] = 0
        kept["age"] += 1
        return kept["cands"]

    def mine_negatives(self, Xi, Xv, item_fields, n_draw, n_neg=1, candidates=None, exclude=None, generator=None, refresh_every=1):
        """Hard negatives for every positive row (fmx.pairwise.mine_negatives): n_draw candidates drawn per row, scored under the
        current FM, the n_neg best kept that are neither the row's own item nor excluded -> (items int64 [B, n_neg, m] in the
        order of item_fields, scores fp32 [B, n_neg]) on the device, what fit_pairs takes as negatives.  candidates: [N, m]
        items (None: every row of the one item field); exclude: per-row candidate positions (fmx.recommend.exclusions_csr).
        The candidates are scored with value 1 in the item columns: a positive whose item Xv is not 1 is mined under that
        approximation.  The draws are Philox4x32-10 under seed = generator.initial_seed() (no generator: the attribute
        mining_seed) and offset = the model's count of mining calls, which pickling carries: the same model state, seed and
        call number give the same negatives.  A row with fewer than n_neg eligible draws repeats its best one; a row with none
        at all raises ValueError (one host read per call)."""
        if self._logit_family != "fm":
            self._refuse_hard_negatives("mine_negatives", "hard")
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        fields = self._item_fields(item_fields)
        cands = self._mining_candidates(fields, candidates, refresh_every)
        own = cands.positions_of(idx_d[:, fields], fields)
        seed, offset = self._next_draw(generator)
        pos, score = fmx.pairwise.mine_negatives(self._table, cands, idx_d, xv_d, own, int(n_draw), int(n_neg), seed=seed,
                                                 offset=offset, exclude=exclude, hyper=self._hyper)
        missing = pos < 0
        if bool(missing[:, 0].any()):
            raise ValueError(f"{self._name}.mine_negatives: a row has no eligible candidate among its {int(n_draw)} draws "
                             "(every draw was its own item, excluded or scored NaN)")
        pos = torch.where(missing, pos[:, :1], pos).long()
        score = torch.where(missing, score[:, :1], score)
        items = cands.idx[pos.reshape(-1)][:, cands.item_fields].long()
        items = items[:, [cands.item_fields.index(f) for f in fields]].reshape(pos.shape[0], pos.shape[1], len(fields))
        return items, score


class NetworkPairTraining:
    """DeepFMAdam's and NFMAdam's fit_pairs / run_pair_experiment: RankingTraining's, with the keyword full.  full=False is the
    pure FM's refusal (the pair loss of fmx_fm_pair_* is the pure FM logit's); full=True -- the word recommend / rank use for
    the whole network -- trains on the pair loss of the logit forward() returns (fmx_mlp_pair_section).  Listed in front of
    OnlineFMBase in the class's bases."""

    # run_pair_experiment(full=True) on the device (fmx_online_run_mlp_pair) where _pair_device_loop_ok() says so.  Off by
    # default: the host loop of section calls stays the class's own path; set it to True on an instance (or the class).
    pair_loop_on_device = False

    def _pair_device_loop_ok(self):
        """Can run_pair_experiment(full=True)'s predict-then-fit loop run on the device for this model?  Under 'signadam' / 'sgd',
        and under 'adam' / 'adagrad' with fused_optimizer=True (the hidden layers' flat moments; 'ftrl' and the torch optimizer
        of fused_optimizer=False stay on the host loop), where the one-workgroup MLP step takes the network at two rows.
        The device loop then follows fmx_mlp_pair_fit's arithmetic -- the one-workgroup kernel's summation order -- while the host
        loop keeps fmx_mlp_pair_section at every batch size: the two differ at one pair in the order of fp32 summations only, so
        a stream through either agrees to rounding, not bit for bit."""
        rule = self.update_rule
        if not (rule in ("signadam", "sgd") or (rule in ("adam", "adagrad") and getattr(self, "_mlp_fused", None) is not None)):
            return False
        return self._engine.mlp_fits(2, self.embedding_size, self.neuron_per_hidden_layer, self.num_hidden_layers, "fit")

    def _fit_pairs_full(self, Xi, Xv, item_fields, negatives, n_neg, margin, candidates, generator):
        """fit_pairs(full=True): forward with no loss, the MLP section under the pair loss on bi (fmx_mlp_pair_section), sort,
        table update with dz (and dz again for the FM term where forward() has it) and gbi.  The network's rule follows _fit's
        native branches: 'sgd' inside the section's reduction, 'signadam' (and 'ftrl', whose hidden layers _fit also gives the
        fresh Adam) the closed form p -= lr g / (|g| + 1e-8) on the flat gradients, 'adam' / 'adagrad' the model's fused
        optimizer state.  Every batch size goes through the section."""
        rule = self.update_rule
        if rule in ("adam", "adagrad") and getattr(self, "_mlp_fused", None) is None:
            raise ValueError(f"{self._name}.fit_pairs(full=True) under update_rule={rule!r} trains the hidden layers inside the MLP "
                             "section: construct the model with fused_optimizer=True")
        self.train()
        rows, xv = self._pair_rows(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)
        e, k, lr = self._engine, self.embedding_size, float(self.n)
        B2 = e.forward(self._hyper, rows, xv)
        P = B2 // 2
        if getattr(self, "_mlp_gflat", None) is None:
            self._mlp_gflat = torch.zeros_like(self._mlp_flat)
        loss, dz, gbi, _ = e.mlp_pair_section(self._mlp_flat, self._mlp_gflat, k, self.neuron_per_hidden_layer, self.num_hidden_layers,
                                              e.bi[:B2], self._base_logit(B2).contiguous(), P, 1.0 / P, margin=margin,
                                              lr_apply=lr if rule == "sgd" else 0.0, mlp_opt=self._mlp_fused)
        if rule in ("signadam", "ftrl"):
            g = self._mlp_gflat
            with torch.no_grad():
                self._mlp_flat.sub_(lr * g / (g.abs() + 1e-8))
        e.sort(rows)
        e.update(self._hyper, rule, B2, xv, dz, dz if self._fm_term_in_forward else None, gbi, inv_b=1.0 / P, with_loss=False)
        out = loss[0].clone()
        self._after_step()
        return out

    def fit_pairs(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None, full=False):
        """RankingTraining.fit_pairs's arguments; full=True: one mini-batch pair step of tables and network on the logit forward()
        returns, under the model's update rule ('adam' / 'adagrad' need fused_optimizer=True).  Returns the mean pair loss."""
        self._refuse_hard_negatives("fit_pairs", negatives)
        if not full:
            self._pure_fm_only("fit_pairs", own=("full", "the whole network's"))
        return self._fit_pairs_full(Xi, Xv, item_fields, negatives, n_neg, margin, candidates, generator)

    def run_pair_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=1, margin=0.0, candidates=None, generator=None, full=False):
        """RankingTraining.run_pair_experiment's arguments and 4-tuple; full=True: predict z_pos > z_neg through the whole network,
        then fit_pairs(full=True) on that pair alone, pair by pair -- the host loop of one-pair section calls (pair i's prediction
        is z_pos > z_neg of that step's own logits, the whole network's before its update), or, with the attribute
        pair_loop_on_device set to True, one call of fmx_online_run_mlp_pair where _pair_device_loop_ok() says so (its docstring:
        which models, and with which arithmetic)."""
        self._refuse_hard_negatives("run_pair_experiment", negatives)
        if not full:
            self._pure_fm_only("run_pair_experiment", own=("full", "the whole network's"))
        start = time()
        self.train()
        rows, xv = self._pair_rows(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)
        n, e = rows.shape[0] // 2, self._engine
        if n == 0:
            return self._experiment_result(start, None)
        if self.pair_loop_on_device and self._pair_device_loop_ok():
            pred = e.online_run_mlp_pair(self._hyper, self.update_rule, self._mlp_flat, self.embedding_size, self.neuron_per_hidden_layer,
                                         self.num_hidden_layers, self._fm_term_in_forward, rows, xv, margin=margin,
                                         mlp_opt=getattr(self, "_mlp_fused", None))[0]
            return self._experiment_result(start, pred)
        fields = self._item_fields(item_fields)

        def fit_one(i):
            pos, pos_xv, neg = self._pair_at(rows, xv, fields, i)
            self._fit_pairs_full(pos, pos_xv, fields, neg, 1, margin, None, None)
        return self._experiment_result(start, self._host_stream_loop(n, fit_one, lambda: e._mlp_logit[0] > e._mlp_logit[1]))


class NetworkListTraining:
    """DeepFMAdam's and NFMAdam's fit_lists / run_list_experiment: RankingTraining's, with the keyword full.  full=False is the
    pure FM's refusal, raised before any state is read (the list loss of fmx_fm_list_* is the pure FM logit's); full=True trains on
    the list loss of the logit forward() returns (fmx_mlp_list_section).  Listed beside NetworkPairTraining, in front of
    OnlineFMBase, in the class's bases."""

    # run_list_experiment(full=True) on the device (fmx_online_run_mlp_list) where _list_device_loop_ok() says so.  Off by
    # default: the host loop of section calls stays the class's own path; set it to True on an instance (or the class).
    list_loop_on_device = False

    def _list_device_loop_ok(self, G=None):
        """Can run_list_experiment(full=True)'s predict-then-fit loop run on the device for this model (at lists of G rows; None:
        the longest, 16)?  Under 'signadam' / 'sgd', and under 'adam' / 'adagrad' with fused_optimizer=True (the hidden layers'
        flat moments; 'ftrl' and the torch optimizer of fused_optimizer=False stay on the host loop), where the one-workgroup MLP
        step takes the network at G rows and the table is one fmx_fm_list_online_run takes (FMEngine.list_online_run_fits: the
        fields fit one wavefront's passes, plain fields, no sort split).
        The device loop then follows fmx_mlp_list_fit's arithmetic -- the one-workgroup kernel's summation order -- while the host
        loop keeps fmx_mlp_list_section at every batch size: the two differ at one list in the order of fp32 summations only, so
        a stream through either agrees to rounding, not bit for bit."""
        rule = self.update_rule
        if not (rule in ("signadam", "sgd") or (rule in ("adam", "adagrad") and getattr(self, "_mlp_fused", None) is not None)):
            return False
        e = self._engine
        G = fmx._lib.LIST_MAX_G if G is None else int(G)
        return (e.mlp_fits(G, self.embedding_size, self.neuron_per_hidden_layer, self.num_hidden_layers, "fit")
                and e.list_online_run_fits(self.field_size, self._table.kp))

    def _fit_lists_full(self, Xi, Xv, item_fields, negatives, n_neg, candidates, generator):
        """fit_lists(full=True), the list mirror of _fit_pairs_full: the lists' rows, forward with no loss, the MLP section under
        the list loss on bi (fmx_mlp_list_section, inv_b = 1 / lists; the sampler's log Q as its corr under
        PopularityNegatives(correct=True)), the network's rule by _fit_pairs_full's branches, sort, and the table update with dz
        (and dz again for the FM term where forward() has it) and gbi on the list steps' copy of the table, whose bias rule runs
        on scratch: the bias does not move.  Every batch size goes through the section."""
        rule = self.update_rule
        if rule in ("adam", "adagrad") and getattr(self, "_mlp_fused", None) is None:
            raise ValueError(f"{self._name}.fit_lists(full=True) under update_rule={rule!r} trains the hidden layers inside the MLP "
                             "section: construct the model with fused_optimizer=True")
        self.train()
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        popular = fmx.pairwise.popularity_negatives(negatives)
        corr = None
        if popular is not None and popular.correct:
            negatives, corr = self._sample_popular(idx_d, self._item_fields(item_fields), popular, n_neg, candidates, generator)
        rows, xv, G = self._list_rows("fit_lists", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
        e, k, lr = self._engine, self.embedding_size, float(self.n)
        N = e.forward(self._hyper, rows, xv)
        B = N // G
        if getattr(self, "_mlp_gflat", None) is None:
            self._mlp_gflat = torch.zeros_like(self._mlp_flat)
        loss, dz, gbi, _ = e.mlp_list_section(self._mlp_flat, self._mlp_gflat, k, self.neuron_per_hidden_layer, self.num_hidden_layers,
                                              e.bi[:N], self._base_logit(N).contiguous(), B, G, 1.0 / B,
                                              corr=None if corr is None else corr.reshape(-1),
                                              lr_apply=lr if rule == "sgd" else 0.0, mlp_opt=self._mlp_fused)
        if rule in ("signadam", "ftrl"):
            g = self._mlp_gflat
            with torch.no_grad():
                self._mlp_flat.sub_(lr * g / (g.abs() + 1e-8))
        e.list_sort_update(self._hyper, rule, rows, G, xv, dz, dz if self._fm_term_in_forward else None, gbi, inv_b=1.0 / B)
        out = loss[0].clone()
        self._after_step()
        return out

    def _list_full_checks(self, method, negatives, n_neg):
        """What fit_lists / run_list_experiment(full=True) refuse before the model is looked at: mined negatives (they are mined
        under the pure FM score), and a count of drawn negatives outside 1 .. 15"""
        self._refuse_hard_negatives(method, negatives)
        if negatives is None or fmx.pairwise.popularity_negatives(negatives) is not None:
            self._list_limit(method, n_neg)

    def fit_lists(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, full=False):
        """RankingTraining.fit_lists's arguments; full=True: one mini-batch list step of tables and network on the logit forward()
        returns, under the model's update rule ('adam' / 'adagrad' need fused_optimizer=True).  negatives: given arrays, None
        (uniform draws) or a fmx.pairwise.PopularityNegatives -- with its correct=True the softmax runs on logit - log Q;
        "hard" / a HardNegatives is refused by name.  Returns the mean list loss; the bias does not move."""
        if not full:
            self._pure_fm_only("fit_lists", "list")
        self._list_full_checks("fit_lists", negatives, n_neg)
        return self._fit_lists_full(Xi, Xv, item_fields, negatives, n_neg, candidates, generator)

    def run_list_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, full=False):
        """RankingTraining.run_list_experiment's arguments and 4-tuple; full=True: for every positive and its negatives predict the
        positive's rank among that step's own whole-network logits (the uncorrected ones, before the update; correct: no negative
        scores as high as the positive), then fit_lists(full=True) on that list alone -- the host loop of one-list section calls.
        A PopularityNegatives draws every list's negatives in its own call, as the pure FM's loop does.
        With the attribute list_loop_on_device set to True: one call of fmx_online_run_mlp_list where _list_device_loop_ok() says
        so (its docstring: which models, and with which arithmetic -- the one-workgroup kernel's summation order, so it agrees
        with the host loop to rounding, not bit for bit).  A PopularityNegatives then draws the negatives of ALL positives in
        one sampler call up front, which consumes the generator differently from the host loop's per-list draws: the same law,
        other draws; with its correct=True the draws' log Q is the call's corr."""
        if not full:
            self._pure_fm_only("run_list_experiment", "list")
        self._list_full_checks("run_list_experiment", negatives, n_neg)
        start = time()
        self.train()
        idx_d, xv_d, _ = self._inputs(Xi, Xv)
        n, e = idx_d.shape[0], self._engine
        if n == 0:
            return self._experiment_result(start, None)
        popular = fmx.pairwise.popularity_negatives(negatives)
        if self.list_loop_on_device and self._list_device_loop_ok():
            corr = None
            if popular is not None:
                negatives, corr = self._sample_popular(idx_d, self._item_fields(item_fields), popular, n_neg, candidates, generator)
            rows, xv, G = self._list_rows("run_list_experiment", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
            ranks = e.online_run_mlp_list(self._hyper, self.update_rule, self._mlp_flat, self.embedding_size, self.neuron_per_hidden_layer,
                                          self.num_hidden_layers, self._fm_term_in_forward, rows, G, xv,
                                          corr=corr.reshape(-1) if corr is not None and popular.correct else None,
                                          mlp_opt=getattr(self, "_mlp_fused", None))[0]
            return self._experiment_result(start, ranks == 0)
        if popular is not None:
            G = 1 + int(n_neg)
            whole = popular.exclude
            off, pos = fmx.recommend.exclusions_csr(whole, n, "cpu")

            def fit_one(i):
                if off is not None:
                    popular.exclude = (off[i:i + 2] - off[i], pos[int(off[i]):int(off[i + 1])])
                self._fit_lists_full(idx_d[i:i + 1], None if xv_d is None else xv_d[i:i + 1], item_fields, popular, n_neg, candidates,
                                     generator)
        else:
            whole = None
            rows, xv, G = self._list_rows("run_list_experiment", idx_d, xv_d, item_fields, negatives, n_neg, candidates, generator)
            fields = self._item_fields(item_fields)

            def fit_one(i):
                lst = rows[G * i:G * (i + 1)]
                self._fit_lists_full(lst[:1], None if xv is None else xv[G * i:G * i + 1], fields, lst[1:, fields].reshape(1, G - 1, -1),
                                     G - 1, None, None)
        try:
            ranks = self._host_stream_loop(n, fit_one, lambda: (e._mlp_logit[1:G] >= e._mlp_logit[0]).sum())
        finally:
            if popular is not None:
                popular.exclude = whole
        return self._experiment_result(start, ranks == 0)


class NetworkListRefused:
    """DeepFMOnn's and NFMOnn's fit_lists / run_list_experiment: the signature of NetworkListTraining, and RankingTraining's
    refusal under full as well -- Hedge backprop has a loss per layer, and no list form of it is built."""

    def fit_lists(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, full=False):
        self._pure_fm_only("fit_lists", "list")

    def run_list_experiment(self, Xi, Xv, item_fields, negatives=None, n_neg=4, candidates=None, generator=None, full=False):
        self._pure_fm_only("run_list_experiment", "list")
