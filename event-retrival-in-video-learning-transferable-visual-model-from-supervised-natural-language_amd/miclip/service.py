"""``EmbeddingService`` with the reference's interface, ranking on the GPU.

Mirror of ``Backend/services/embedding_service.py:69-536`` — same constructor
(injected cache/path/data services), same method names, arguments, return
types and swallow-to-``[]``/``0.0`` error semantics (:280-282, :342-344), so
``Backend/app.py`` and ``Backend/query_strategies.py`` (which receive
``search_top_frames`` / ``extract_query_confidence`` as callables,
app.py:157-174) work unchanged.  What moves to the device:

  get_text_features      clip.tokenize -> encode_text (+L2 in the kernel)      :151-184
  search_top_frames      np.dot + np.argsort(s)[::-1][:k] -> one fused kernel  :284-344
                         over the HBM-resident corpus (file rows, normalised
                         as get_embeddings does at load :209-210: f32 files
                         in the rank kernel; float16 files -- the reference's
                         default video_test_3 / image_embeddings.npy -- by
                         mi_normalize_rows_f16 in NumPy's float16 arithmetic,
                         then ranked as stored)
  search_top_frames_by_image                                                    :346-392
  extract_and_save_embeddings_from_folder  batches -> encode_image (+L2)      :425-536

The frame list (row order) still comes from ``data_service.load_frames_from_json``
(data_service.py:48), and ``get_embeddings`` keeps returning the normalised
numpy array other callers (visualization_service) expect.
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import api
from .preprocess import decode_chunk, load_frames
from .library import FrameLibrary
from .retrieval import (MirroredCorpus, collapse_topk, event_topk, exclude_similar, normalize_rows_f16, rank_topk,
                        rank_topk_distinct, score_matrix)

# corpora from this many rows on also get an fp16 ranking mirror (scripts/mirror_micro.py:
# 1M rows 1.6-1.9x faster than the exact pass, 125k rows slower: fixed merge/re-score cost)
MIRROR_MIN_ROWS = 262_144
from .weights import load_classifier, load_state_dict


def frame_time_order(frames):
    """A frames list -> (times, order).  times: int64 [n], the frame numbers the reference reads
    from the file names (``int(Path(frame_name).stem)``, query_strategies.py:74), or None when some
    stem is not an integer (then time is the row number).  order: int64 [n], the rows in time
    order, a stable sort (rows of equal time keep their row order); the identity without times.
    Frame lists come string-sorted ("10152.jpg" before "2214.jpg"), so the two orders differ."""
    n = len(frames)
    try:
        stems = [os.path.splitext(os.path.basename(str(f)))[0] for f in frames]
        if not all(st.isascii() and st.isdigit() for st in stems):
            raise ValueError
        times = np.array([int(st) for st in stems], dtype=np.int64).reshape(n)
    except (ValueError, OverflowError):
        return None, np.arange(n, dtype=np.int64)
    return times, np.argsort(times, kind="stable").astype(np.int64)


def gemm_f32(a, w, bias=None, relu=False):
    """f32 [M,K] . [N,K]^T (+bias) (+ReLU) through ``mi_op_gemm_f32`` (the fp32
    tower's exact-f32 MFMA GEMM); K is zero-padded to a multiple of 32."""
    import torch
    from . import _native as N
    a = a.float().contiguous()
    w = w.float().contiguous()
    M, K = a.shape
    Nn = w.shape[0]
    if K % 32:
        pad = 32 - K % 32
        a = torch.nn.functional.pad(a, (0, pad))
        w = torch.nn.functional.pad(w, (0, pad))
        K += pad
    out = torch.empty(M, Nn, dtype=torch.float32, device=a.device)
    if M == 0:
        return out
    b = bias.float().contiguous() if bias is not None else None
    with torch.cuda.device(a.device):
        N.check(N.lib().mi_op_gemm_f32(a.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                       out.data_ptr(), M, Nn, K, 3 if relu else 0, N.stream_ptr(a.device)),
                "mi_op_gemm_f32")
    return out


class FinetunedCLIP:
    """``CLIPWithClassifier`` (embedding_service.py:16-67) on the device:
    ``clip_model.float()`` (:22, the fp32 tower), ``model(images)`` = L2-normalised
    image features (:36-49); with texts, the CLIP logits (logit_scale.exp() *
    I . T^T) and the 3-class head Linear(D, 512) -> ReLU -> Dropout (identity at
    inference) -> Linear(512, 3) on the checkpoint's ``classifier.*`` weights
    (:51-67)."""

    def __init__(self, clip_model, classifier=None):
        import torch
        self.clip_model = clip_model.float()
        self.logit_scale = clip_model.logit_scale
        self.classifier = None
        if classifier is not None:
            dev = self.clip_model.device
            self.classifier = {k: torch.from_numpy(v).to(dev) for k, v in classifier.items()}

    def __call__(self, images, texts=None, get_embeddings=False):
        import torch
        if texts is not None and self.classifier is None:
            # checked before any encode: the reference's CLIPWithClassifier always has the head
            raise ValueError("this checkpoint has no classifier.* weights: class logits are unavailable")
        image_features = self.clip_model.encode_image(images, normalize=True, out_dtype=torch.float32)
        if texts is None:
            return image_features
        text_features = self.clip_model.encode_text(texts, normalize=True, out_dtype=torch.float32)
        from .retrieval import score_matrix
        scale = float(np.exp(np.float32(self.logit_scale.item())))
        # (logit_scale * image_features) @ text_features.t()  (:57-58)
        logits_per_image = score_matrix(text_features, image_features * scale, norm="none")
        logits_per_text = logits_per_image.t()
        c = self.classifier
        hidden = gemm_f32(image_features, c["0.weight"], c["0.bias"], relu=True)
        class_logits = gemm_f32(hidden, c["3.weight"], c["3.bias"])
        if get_embeddings:
            return image_features, text_features, logits_per_image, logits_per_text, class_logits
        return logits_per_image, logits_per_text, class_logits

    def eval(self):
        return self

    def to(self, device):
        self.clip_model.to(device)
        return self


class EmbeddingService:
    def __init__(self, cache_service, path_service, data_service, device="cuda", model_name="ViT-B/32",
                 checkpoint_path=None):
        self.cache_service = cache_service
        self.path_service = path_service
        self.data_service = data_service
        self.device = device
        self.model_name = model_name
        self.original_model, self.preprocess = api.load(model_name, device=device)
        self.finetuned_model = None
        self.active_model = "original"
        self.checkpoint_path = checkpoint_path or os.environ.get("CLIP_FINETUNED_CHECKPOINT", "")
        self._device_corpus = {}
        self._mirrors = {}          # id(device corpus) -> MirroredCorpus (large corpora)
        self._library = None        # (video names, embedding paths, mtimes, FrameLibrary)
        self._lookup = {}
        if self.checkpoint_path and os.path.exists(self.checkpoint_path):
            try:
                self._load_finetuned_model(self.checkpoint_path)
            except Exception as e:  # reference: print and continue (:98-99)
                print(f"Error loading finetuned model: {e}")

    # ----------------------------------------------------------- model state
    def _load_finetuned_model(self, checkpoint_path):
        sd = load_state_dict(checkpoint_path)       # unwraps model_state_dict / clip_model.*
        model, _ = api.load(self.model_name, device=self.device)
        model.load_state_dict(sd)
        self.finetuned_model = FinetunedCLIP(model, load_classifier(checkpoint_path))

    def set_active_model(self, model_name):
        if model_name == "original":
            self.active_model = "original"
            return True
        if model_name == "finetuned":
            if self.finetuned_model is not None:
                self.active_model = "finetuned"
                return True
            return False
        return False

    def get_active_model_name(self):
        return self.active_model

    def _clip(self):
        if self.active_model == "finetuned" and self.finetuned_model is not None:
            return self.finetuned_model.clip_model
        return self.original_model

    # ------------------------------------------------------------- features
    def get_text_features(self, query, video_name=None):
        cache_key = f"{self.active_model}_{query}_{video_name or 'default'}"
        features = self.cache_service.get_text_features(cache_key, video_name)
        if features is not None:
            return features
        tokens = api.tokenize([query])
        feats = self._clip().encode_text(tokens, normalize=True, out_dtype=__import__("torch").float32)
        features = feats.cpu().numpy()
        self.cache_service.set_text_features(cache_key, video_name, features)
        return features

    def get_embeddings(self, video_name=None):
        embeddings_path = self.path_service.get_embeddings_path(video_name)
        embeddings = self.cache_service.get_embeddings(embeddings_path)
        if embeddings is not None:
            return embeddings
        if not os.path.exists(embeddings_path):
            print(f"Warning: Embeddings file not found: {embeddings_path}")
            return None
        try:
            embeddings = np.load(embeddings_path)
            embeddings = embeddings / np.linalg.norm(embeddings, axis=-1, keepdims=True)
            self.cache_service.set_embeddings(embeddings_path, embeddings)
            return embeddings
        except Exception as e:
            print(f"Error loading embeddings: {e}")
            return None

    def _corpus_on_device(self, video_name):
        """(rows, norm) resident in HBM for the rank kernel, normalised as
        get_embeddings normalises the file (embedding_service.py:209-210):
        f32 rows stay raw and the rank kernel normalises each row in the same
        pass (norm "l2"); float16 rows -- NumPy normalises those in float16 --
        are normalised once on the device bit for bit as NumPy does it
        (``normalize_rows_f16``) and ranked as they are (norm "none"), so
        search_top_frames ranks exactly the rows extract_query_confidence
        reads from get_embeddings."""
        import torch
        path = self.path_service.get_embeddings_path(video_name)
        if not os.path.exists(path):
            return None
        mtime = os.path.getmtime(path)
        hit = self._device_corpus.get(path)
        if hit is not None and hit[0] == mtime:
            return hit[1]
        if hit is not None:
            self._mirrors.pop(id(hit[1][0]), None)   # the file changed: drop the old rows' mirror
        raw = np.load(path)
        if raw.dtype not in (np.float32, np.float16):
            raw = raw.astype(np.float32)
        t = torch.from_numpy(np.ascontiguousarray(raw)).to(self.original_model.device)
        if t.dtype == torch.float16:
            entry = (normalize_rows_f16(t, out=t), "none")
        else:
            entry = (t, "l2")
            if t.shape[0] >= MIRROR_MIN_ROWS and t.shape[1] in (512, 768):
                self._mirrors[id(t)] = MirroredCorpus(t)
        self._device_corpus[path] = (mtime, entry)
        return entry

    def _frames(self, video_name):
        json_path = self.path_service.get_metadata_path(video_name)
        frames = self.cache_service.get_frames_list(json_path)
        if frames is None:
            frames = self.data_service.load_frames_from_json(video_name)
            self.cache_service.set_frames_list(json_path, frames)
        return frames

    def _rank(self, entry, query_vec, top_k):
        """Top-k (score desc, index asc; NaN first as argsort(s)[::-1]); any
        k up to the corpus size (a full sort when top_k >= N, as the reference's
        np.argsort(s)[::-1] at embedding_service.py:317-318).  ``entry`` is
        ``_corpus_on_device``'s (rows, norm)."""
        import torch
        corpus, norm = entry
        k = min(int(top_k), corpus.shape[0])
        if k <= 0:
            return np.zeros(0, np.float32), np.zeros(0, np.int64)
        q = torch.as_tensor(np.asarray(query_vec, dtype=np.float32).reshape(1, -1), device=corpus.device)
        mc = self._mirrors.get(id(corpus))
        if mc is not None and mc.master is corpus and norm == "l2" and k <= MirroredCorpus.MAX_K:
            s, i = mc.topk(q, k, norm="l2", nan_policy="first")   # certified == the exact pass, bit for bit
        else:
            s, i = rank_topk(corpus, q, k, norm=norm, nan_policy="first")
        return s[0].cpu().numpy(), i[0].cpu().numpy()

    # --------------------------------------------------------------- search
    def extract_query_confidence(self, frame_path, query, video_name=None):
        try:
            text_features = self.get_text_features(query, video_name)
            embeddings = self.get_embeddings(video_name)
            if embeddings is None:
                return 0.0
            frames = self._frames(video_name)
            cached = self._lookup.get(id(frames))
            if cached is None or cached[0] is not frames:
                # first occurrence wins, as list.index (embedding_service.py:264-271)
                by_path = {f: i for i, f in reversed(list(enumerate(frames)))}
                by_name = {os.path.basename(f): i for i, f in reversed(list(enumerate(frames)))}
                cached = (frames, by_path, by_name)
                self._lookup[id(frames)] = cached
            index = cached[1].get(frame_path)
            if index is None:
                index = cached[2].get(os.path.basename(frame_path))
                if index is None:
                    return 0.0
            return float(np.dot(embeddings[index:index + 1], text_features.T)[0][0])
        except Exception as e:
            print(f"Error extracting query confidence: {e}")
            return 0.0

    def search_top_frames(self, query, top_k, video_name=None):
        try:
            cache_key = f"search_{self.active_model}_{query}_{top_k}"
            cached = self.cache_service.get_search_results(cache_key, video_name)
            if cached is not None:
                return cached
            text_features = self.get_text_features(query, video_name)
            corpus = self._corpus_on_device(video_name)
            if corpus is None:
                return []
            _, idx = self._rank(corpus, text_features, top_k)
            frames = self._frames(video_name)
            top_frames = [frames[i] for i in idx]
            self.cache_service.set_search_results(cache_key, video_name, top_frames)
            return top_frames
        except Exception as e:
            print(f"Error in search_top_frames: {e}")
            return []

    def _frame_library(self, video_names):
        """One resident ``FrameLibrary`` over the videos' embedding files, rebuilt when the
        list of videos or a file's mtime changes (``_corpus_on_device``'s invalidation);
        None when a file is missing."""
        names = tuple(video_names)
        paths = tuple(self.path_service.get_embeddings_path(v) for v in names)
        if not all(os.path.exists(p) for p in paths):
            return None
        mtimes = tuple(os.path.getmtime(p) for p in paths)
        hit = self._library
        if hit is not None and hit[:3] == (names, paths, mtimes):
            return hit[3]
        lib = FrameLibrary(device=self.original_model.device)
        for v, p in zip(names, paths):
            rows = np.load(p)
            # frame numbers as the time axis of search_events_all, where every stem is one
            times = frame_time_order(self._frames(v))[0]
            if times is not None and (times.shape[0] != rows.shape[0] or (times >= 1 << 40).any()):
                times = None
            lib.add(v, rows, times=times)
        self._library = (names, paths, mtimes, lib)
        return lib

    @staticmethod
    def _allow_rows(frames, allow_frames):
        """``allow_frames`` (video -> frame basenames) as ``FrameLibrary``'s allow dict (video ->
        row numbers); None stays None."""
        if allow_frames is None:
            return None
        allow = {}
        for v, wanted in allow_frames.items():
            if v not in frames:
                continue
            wanted = {os.path.basename(f) for f in wanted}
            allow[v] = np.array([i for i, f in enumerate(frames[v]) if os.path.basename(f) in wanted],
                                dtype=np.int64)
        return allow

    def search_top_frames_all(self, query, top_k, video_names, allow_frames=None):
        """``search_top_frames`` over several videos at once (the UI's "all videos" filter,
        app.py:402-429, 567-588, 605): ``[(video_name, frame), ...]``, best first, from one
        filtered pass over the resident library (at most ``top_k`` <= 64 entries).
        ``allow_frames``: optional dict video -> iterable of frame basenames (what
        ``search_frames_by_keyword`` returns); then only those frames are ranked -- the exact
        form of the hybrid strategies' "CLIP top_k*3, then intersect" -- and a video absent
        from the dict is excluded.  Errors are swallowed to ``[]`` as in ``search_top_frames``."""
        try:
            video_names = list(video_names)
            if not video_names or int(top_k) <= 0:
                return []
            lib = self._frame_library(video_names)
            if lib is None:
                return []
            frames = {v: self._frames(v) for v in video_names}
            allow = self._allow_rows(frames, allow_frames)
            text_features = self.get_text_features(query, None)
            k = min(int(top_k), max(len(lib), 1))
            _, vid, row = lib.search(np.asarray(text_features, dtype=np.float32).reshape(1, -1), k, allow=allow)
            vid, row = vid[0].cpu().numpy(), row[0].cpu().numpy()
            return [(lib.names[v], frames[lib.names[v]][r]) for v, r in zip(vid, row) if v >= 0]
        except Exception as e:
            print(f"Error in search_top_frames_all: {e}")
            return []

    def search_top_frames_by_image(self, image_features, top_k, video_name=None):
        try:
            corpus = self._corpus_on_device(video_name)
            if corpus is None:
                return []
            _, idx = self._rank(corpus, np.asarray(image_features, dtype=np.float32).reshape(-1), top_k)
            frames = self._frames(video_name)
            return [frames[i] for i in idx]
        except Exception as e:
            print(f"Error in search_top_frames_by_image: {e}")
            return []

    # ------------------------------------------------------------- distinct
    def _rank_distinct(self, video_name, query_vec, top_k, similarity, pool, with_groups, fill=False):
        """The top-k distinct frames of one video: ``_rank`` for the pool (the mirror when it
        applies), ``collapse_topk`` over the resident rows, then the frame mapping.
        ``fill``: ``rank_topk_distinct(fill=True)`` over the resident rows instead."""
        import torch
        entry = self._corpus_on_device(video_name)
        if entry is None:
            return None
        corpus = entry[0]
        k = min(int(top_k), 64, corpus.shape[0])
        if k <= 0:
            return []
        pool = min(64, 3 * k) if pool is None else int(pool)
        pool = min(max(pool, k), 64, corpus.shape[0])
        if fill:
            return self._rank_distinct_filled(video_name, entry, query_vec, k, float(similarity), pool, with_groups)
        s, idx = self._rank(entry, query_vec, pool)
        s = torch.from_numpy(np.ascontiguousarray(s)).reshape(1, -1)
        idx = torch.from_numpy(np.ascontiguousarray(idx)).reshape(1, -1)
        _, hit, _, slot = collapse_topk(corpus, s, idx, k, float(similarity))
        hit, slot = hit[0].cpu().numpy(), slot[0].cpu().numpy()
        frames = self._frames(video_name)
        idx = idx[0].numpy()
        if not with_groups:
            return [frames[i] for i in hit if i >= 0]
        return [(frames[i], [frames[j] for j in idx[slot == s] if j != i]) for s, i in enumerate(hit) if i >= 0]

    def _rank_distinct_filled(self, video_name, entry, query_vec, k, similarity, pool, with_groups):
        """``_rank_distinct`` through the refill rounds.  A hit's group is recovered with one
        single-hit ``exclude_similar`` per hit, chained in slot order: the bits it clears
        (mask before XOR mask after) are the frames of the video collapsed into that hit.
        Round 1 is ``rank_topk_distinct``'s exact pass, not ``_rank``: a video large enough for
        the fp16 mirror (certified, so the same result) pays the slower pool pass here."""
        import torch
        corpus, norm = entry
        q = torch.as_tensor(np.asarray(query_vec, dtype=np.float32).reshape(1, -1), device=corpus.device)
        _, hit, _ = rank_topk_distinct(corpus, q, k, similarity, pool=pool, fill=True, norm=norm, nan_policy="first")
        hit = [i for i in hit[0].tolist() if i >= 0]   # one host read
        frames = self._frames(video_name)
        if not with_groups:
            return [frames[i] for i in hit]
        n = corpus.shape[0]
        mask, masks = None, []
        for i in hit:
            mask, _ = exclude_similar(corpus, corpus[i:i + 1], [i], similarity, row_mask=mask)
            masks.append(mask)
        prev = np.full((n + 31) // 32, -1, np.int32)
        out = []
        for i, m in zip(hit, torch.stack(masks).cpu().numpy()):
            gone = np.unpackbits((prev ^ m).view(np.uint8), bitorder="little")[:n]
            out.append((frames[i], [frames[j] for j in np.flatnonzero(gone) if j != i]))
            prev = m
        return out

    def search_top_frames_distinct(self, query, top_k, video_name=None, similarity=0.9, pool=None,
                                   with_groups=False, fill=False):
        """``search_top_frames`` for distinct moments: the best ``pool`` frames (default
        ``min(64, 3 top_k)``, the reference's ``top_k * 3`` over-fetch) collapsed where the
        cosine of two stored rows is >= ``similarity``; at most ``top_k`` <= 64 frames, best
        first, each the best-ranked of its group.  ``with_groups=True``: ``[(frame, [the
        pool's frames collapsed into it]), ...]``.  Same caching, frame mapping and
        swallow-to-``[]`` as ``search_top_frames``.
        ``fill=True``: the distinct top-k of the whole video instead of the pool's
        (``rank_topk_distinct(fill=True)``): ``top_k`` frames whenever the video holds that many
        distinct ones, however repetitive its footage.  A group then lists every frame of the
        video collapsed into the hit, in frame order (not only the pool's, in rank order)."""
        try:
            cache_key = f"search_distinct_{self.active_model}_{query}_{top_k}_{similarity}_{pool}_{bool(with_groups)}"
            if fill:
                cache_key += "_fill"
            cached = self.cache_service.get_search_results(cache_key, video_name)
            if cached is not None:
                return cached
            text_features = self.get_text_features(query, video_name)
            out = self._rank_distinct(video_name, text_features, top_k, similarity, pool, with_groups, fill)
            if out is None:
                return []
            self.cache_service.set_search_results(cache_key, video_name, out)
            return out
        except Exception as e:
            print(f"Error in search_top_frames_distinct: {e}")
            return []

    def search_top_frames_by_image_distinct(self, image_features, top_k, video_name=None, similarity=0.9, pool=None,
                                            with_groups=False, fill=False):
        """``search_top_frames_by_image`` with the collapse of ``search_top_frames_distinct``
        (``fill`` included; not cached, as ``search_top_frames_by_image``)."""
        try:
            out = self._rank_distinct(video_name, np.asarray(image_features, dtype=np.float32).reshape(-1), top_k,
                                      similarity, pool, with_groups, fill)
            return [] if out is None else out
        except Exception as e:
            print(f"Error in search_top_frames_by_image_distinct: {e}")
            return []

    # --------------------------------------------------------------- events
    @staticmethod
    def _event_record(frames, peak, begin, end, count, score):
        return {"frame": frames[peak], "start": frames[begin], "end": frames[end], "frames": int(count),
                "score": float(score)}

    def search_events(self, query, top_k, video_name=None, *, threshold, max_gap, min_frames=1, with_total=False):
        """The moments of one video that match ``query``: runs of frames scoring >= ``threshold``
        (the cosine ``extract_query_confidence`` returns; the reference's strategies keep frames
        with ``confidence >= adaptive_threshold``, query_strategies.py:121-186) whose consecutive
        frame numbers differ by at most ``max_gap``, with at least ``min_frames`` frames.  The
        time axis is the frame number in the file name (``frame_time_order``); if some name is not
        a number it is the row number.  ``threshold`` and ``max_gap`` have no defaults: the
        reference's 0.5 is a UI value for another score scale.

        Returns ``[{"frame": best frame, "start": first frame, "end": last frame, "frames": count,
        "score": best score}, ...]``, best first, at most ``top_k`` <= 64; with
        ``with_total=True`` ``(that list, the number of qualifying events)``.  Same caching and
        swallow-to-``[]`` as ``search_top_frames``."""
        empty = ([], 0) if with_total else []
        try:
            import torch
            cache_key = (f"search_events_{self.active_model}_{query}_{top_k}_{float(threshold)}_{int(max_gap)}_"
                         f"{int(min_frames)}_{bool(with_total)}")
            cached = self.cache_service.get_search_results(cache_key, video_name)
            if cached is not None:
                return cached
            text_features = self.get_text_features(query, video_name)
            entry = self._corpus_on_device(video_name)
            if entry is None:
                return empty
            corpus, norm = entry
            k = min(int(top_k), 64)
            if k <= 0 or corpus.shape[0] == 0:
                return empty
            frames = self._frames(video_name)
            times, order = frame_time_order(frames)
            if len(frames) != corpus.shape[0]:
                raise ValueError(f"{len(frames)} frames for {corpus.shape[0]} embedding rows")
            q = torch.as_tensor(np.asarray(text_features, dtype=np.float32).reshape(1, -1), device=corpus.device)
            scores = score_matrix(corpus, q, norm=norm)
            row_time = None
            if times is not None:
                scores = scores.index_select(1, torch.from_numpy(order).to(corpus.device))
                row_time = times[order]
            res = event_topk(scores, float(threshold), k, max_gap=int(max_gap), min_count=int(min_frames),
                             row_time=row_time)
            s, peak, begin, end, count = (t[0].cpu().numpy() for t in res[:5])
            total = int(res[5][0])
            out = [self._event_record(frames, order[p], order[b], order[e], c, v)
                   for v, p, b, e, c in zip(s, peak, begin, end, count) if b >= 0]
            out = (out, total) if with_total else out
            self.cache_service.set_search_results(cache_key, video_name, out)
            return out
        except Exception as e:
            print(f"Error in search_events: {e}")
            return empty

    def search_events_all(self, query, top_k, video_names, *, threshold, max_gap, min_frames=1, allow_frames=None,
                          with_total=False):
        """``search_events`` over several videos at once, from the resident library
        (``FrameLibrary.search_events``): ``[(video_name, record), ...]``, best first; events never
        cross videos.  A video whose frame names are all numbers is on the frame-number axis, any
        other on its row numbers.  ``allow_frames`` is ``search_top_frames_all``'s.  Not cached;
        errors are swallowed to ``[]``."""
        empty = ([], 0) if with_total else []
        try:
            video_names = list(video_names)
            if not video_names or int(top_k) <= 0:
                return empty
            lib = self._frame_library(video_names)
            if lib is None or len(lib) == 0:
                return empty
            frames = {v: self._frames(v) for v in video_names}
            text_features = self.get_text_features(query, None)
            res = lib.search_events(np.asarray(text_features, dtype=np.float32).reshape(1, -1), min(int(top_k), 64),
                                    float(threshold), int(max_gap), min_count=int(min_frames),
                                    allow=self._allow_rows(frames, allow_frames))
            s, vid, peak, begin, end, count = (t[0].cpu().numpy() for t in res[:6])
            out = [(lib.names[v], self._event_record(frames[lib.names[v]], p, b, e, c, x))
                   for x, v, p, b, e, c in zip(s, vid, peak, begin, end, count) if v >= 0]
            return (out, int(res[6][0])) if with_total else out
        except Exception as e:
            print(f"Error in search_events_all: {e}")
            return empty

    # --------------------------------------------------------------- ingest
    def extract_image_embedding(self, image_path):
        try:
            from PIL import Image
            import torch
            image = self.preprocess(Image.open(image_path)).unsqueeze(0)
            if self.active_model == "finetuned" and self.finetuned_model is not None:
                feats = self.finetuned_model(image)
            else:
                feats = self.original_model.encode_image(image, normalize=True, out_dtype=torch.float32)
            return feats.float().cpu().numpy()
        except Exception as e:
            print(f"Error extracting embedding from {image_path}: {e}")
            return None

    def extract_and_save_embeddings_from_folder(self, folder_path, model_name=None, video_name=None,
                                                batch_size=256):
        import torch

        current = self.active_model
        if model_name:
            if model_name == "finetuned" and self.finetuned_model is None:
                model_name = "original"
            self.set_active_model(model_name)
        embeddings_path = self.path_service.get_embeddings_path(video_name)
        os.makedirs(os.path.dirname(embeddings_path) or ".", exist_ok=True)
        frame_files = sorted(f for f in os.listdir(folder_path) if f.endswith((".jpg", ".jpeg", ".png")))
        if not frame_files:
            self.set_active_model(current)
            return None
        model = self._clip()
        R = model.cfg.image_resolution
        out = []
        step = decode_chunk(batch_size)
        for j in range(0, len(frame_files), step):
            # GPU JPEG decode + resize/crop/normalise (Pillow-exact, miclip.preprocess.load_frames) over a
            # large chunk (the decode runs one lane per frame), then the reference's encode batches
            frames, _ = load_frames([os.path.join(folder_path, f) for f in frame_files[j:j + step]], R,
                                    device=model.device)
            for i in range(0, frames.shape[0], batch_size):
                out.append(model.encode_image(frames[i:i + batch_size], normalize=True,
                                              out_dtype=torch.float32).cpu().numpy())
        embeddings = np.vstack(out)
        np.save(embeddings_path, embeddings)
        metadata_path = self.path_service.get_metadata_path(video_name)
        if os.path.exists(metadata_path):
            try:
                with open(metadata_path, "r", encoding="utf-8") as f:
                    metadata = json.load(f)
                if isinstance(metadata, list):
                    for item in metadata:
                        item["embedding_model"] = self.active_model
                elif isinstance(metadata, dict):
                    metadata["embedding_model"] = self.active_model
                with open(metadata_path, "w", encoding="utf-8") as f:
                    json.dump(metadata, f, ensure_ascii=False, indent=2)
            except Exception as e:
                print(f"Error updating metadata with model info: {e}")
        self.set_active_model(current)
        return embeddings_path
