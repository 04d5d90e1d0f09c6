"""The CLIP tokenizer on the host: OpenAI's byte-level BPE and the prompt syntax of the reference's comfy/sd1_clip.py (``(word:1.3)``
weights, ``embedding:<name>`` vectors, sections of 77 tokens).  Self-contained: no transformers, tokenizers or regex package.

The vocabulary is derived from ``merges.txt`` alone (a model resource like weights: ``weights.register_tokenizer`` or
``$SR_MODELS_DIR/tokenizer/merges.txt``): the ids are, in order, the 256 byte symbols, the same 256 with ``</w>``, the first 48 894
merges joined, ``<|startoftext|>`` (49406) and ``<|endoftext|>`` (49407).  Nothing here touches the GPU."""
import functools
import gzip
import os
import unicodedata

import torch

from . import weights as WT

START, END = "<|startoftext|>", "<|endoftext|>"
N_MERGES = 49152 - 256 - 2
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


@functools.lru_cache(maxsize=None)
def bytes_to_unicode():
    """byte -> one of 256 printable code points (the order of the values is the order of the first 256 ids)"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _is_letter(ch):
    return unicodedata.category(ch)[0] == "L"


def _is_number(ch):
    return unicodedata.category(ch)[0] == "N"


def split_words(text):
    """OpenAI's pattern, by hand: the two special tokens | 's 't 're 've 'm 'll 'd | [\\p{L}]+ | [\\p{N}] | [^\\s\\p{L}\\p{N}]+"""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch == "<":
            sp = next((s for s in (START, END) if text.startswith(s, i)), None)
            if sp is not None:
                out.append(sp)
                i += len(sp)
                continue
        if ch == "'":
            # the alternatives in the pattern's own order: 's 't 're 've 'm 'll 'd
            c = next((s for s in _CONTRACTIONS if text.startswith(s, i)), None)
            if c is not None:
                out.append(c)
                i += len(c)
                continue
        if ch.isspace():
            i += 1
        elif _is_letter(ch):
            j = i + 1
            while j < n and _is_letter(text[j]):
                j += 1
            out.append(text[i:j])
            i = j
        elif _is_number(ch):
            out.append(ch)
            i += 1
        else:
            j = i + 1
            while j < n and not (text[j].isspace() or _is_letter(text[j]) or _is_number(text[j])):
                j += 1
            out.append(text[i:j])
            i = j
    return out


def clean(text):
    """NFC, whitespace runs to one space, strip, lower case"""
    return " ".join(unicodedata.normalize("NFC", text).split()).strip().lower()


class BPE:
    """merges.txt -> encode(text) -> ids (without the start and end tokens)"""

    def __init__(self, merges_path=None):
        path = merges_path or WT.tokenizer_merges()
        with (gzip.open if str(path).endswith(".gz") else open)(path, "rt", encoding="utf-8") as f:      # merges.txt or merges.txt.gz
            lines = f.read().strip().split("\n")
        merges = [tuple(m.split()) for m in lines[1:N_MERGES + 1]]
        if len(merges) != N_MERGES or any(len(m) != 2 for m in merges):
            raise ValueError(f"{path}: expected a header line and {N_MERGES} merges of two symbols")
        base = list(bytes_to_unicode().values())
        vocab = base + [v + "</w>" for v in base] + ["".join(m) for m in merges] + [START, END]
        self.encoder = {s: i for i, s in enumerate(vocab)}
        self.decoder = {i: s for s, i in self.encoder.items()}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.start_token, self.end_token = self.encoder[START], self.encoder[END]
        self._cache = {START: START, END: END}

    def __len__(self):
        return len(self.encoder)

    def bpe(self, token):
        if token in self._cache:
            return self._cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = {(a, b) for a, b in zip(word, word[1:])}
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            new, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == a and word[i + 1] == b:
                    new.append(a + b)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = " ".join(word)
        self._cache[token] = out
        return out

    def encode(self, text):
        be = bytes_to_unicode()
        ids = []
        for tok in split_words(clean(text)):
            if tok in (START, END):
                ids.append(self.encoder[tok])
                continue
            sym = "".join(be[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self.bpe(sym).split(" "))
        return ids


# ---- the prompt syntax of sd1_clip.py -------------------------------------------------------------------------------------------------

def parse_parentheses(string):
    result, current, depth = [], "", 0
    for ch in string:
        if ch == "(":
            if depth == 0:
                if current:
                    result.append(current)
                current = "("
            else:
                current += ch
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                result.append(current + ")")
                current = ""
            else:
                current += ch
        else:
            current += ch
    if current:
        result.append(current)
    return result


def token_weights(string, current_weight):
    out = []
    for x in parse_parentheses(string):
        weight = current_weight
        if len(x) >= 2 and x[-1] == ")" and x[0] == "(":
            x = x[1:-1]
            xx = x.rfind(":")
            weight *= 1.1
            if xx > 0:
                try:
                    weight = float(x[xx + 1:])
                    x = x[:xx]
                except ValueError:
                    pass
            out += token_weights(x, weight)
        else:
            out += [(x, current_weight)]
    return out


def escape_important(text):
    return text.replace("\\)", "\0\1").replace("\\(", "\0\2")


def unescape_important(text):
    return text.replace("\0\1", ")").replace("\0\2", "(")


def load_embed(name, embedding_size, embed_key=None):
    """sd1_clip.load_embed: a registered embedding (weights.register_embedding) or a file of $SR_MODELS_DIR/embeddings/ (the name as it
    is, then with .safetensors, .pt, .bin) -> a tensor of one or several vectors, or None.  The legacy zip fallback does not exist."""
    prov = WT._REG["embeddings"].get(WT._norm(name))
    if prov is not None:
        embed = prov()
    else:
        root = os.environ.get("SR_MODELS_DIR")
        if not root:
            return None
        d = os.path.abspath(os.path.join(root, "embeddings"))
        path = os.path.abspath(os.path.join(d, name))
        try:
            if os.path.commonpath((d, path)) != d:
                return None
        except ValueError:
            return None
        if not os.path.isfile(path):
            path = next((path + e for e in (".safetensors", ".pt", ".bin") if os.path.isfile(path + e)), None)
            if path is None:
                return None
        try:
            if path.lower().endswith(".safetensors"):
                from safetensors.torch import load_file
                embed = load_file(path, device="cpu")
            else:
                embed = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:
            return None
    if torch.is_tensor(embed):
        return embed
    if isinstance(embed, list):
        rows = [t.reshape(-1, t.shape[-1]) for d in embed for t in d.values() if t.shape[-1] == embedding_size]
        return torch.cat(rows, dim=0)
    if "string_to_param" in embed:
        return next(iter(embed["string_to_param"].values()))
    if embed_key is not None and embed_key in embed:
        return embed[embed_key]
    return next(iter(embed.values()))


class SDTokenizer:
    """sd1_clip.SDTokenizer.  The BPE (and with it merges.txt) is looked up at the first tokenize call."""

    def __init__(self, max_length=77, pad_with_end=True, embedding_size=768, embedding_key="clip_l", merges_path=None,
                 pad_to_max_length=True, min_length=None):
        self.max_length, self.min_length, self.pad_with_end, self.pad_to_max_length = max_length, min_length, pad_with_end, pad_to_max_length
        self.embedding_size, self.embedding_key, self.merges_path = embedding_size, embedding_key, merges_path
        self.max_word_length = 8
        self.embedding_identifier = "embedding:"
        self._bpe = None

    @property
    def bpe(self):
        if self._bpe is None:
            self._bpe = _shared_bpe(self.merges_path or WT.tokenizer_merges())
        return self._bpe

    @property
    def start_token(self):
        return self.bpe.start_token

    @property
    def end_token(self):
        return self.bpe.end_token

    def _try_get_embedding(self, name):
        embed = load_embed(name, self.embedding_size, self.embedding_key)
        if embed is None:
            stripped = name.strip(",")
            if len(stripped) < len(name):
                return load_embed(stripped, self.embedding_size, self.embedding_key), name[len(stripped):]
        return embed, ""

    def tokenize_with_weights(self, text, return_word_ids=False):
        bpe = self.bpe
        start, end = bpe.start_token, bpe.end_token
        pad = end if self.pad_with_end else 0
        tokens = []
        for segment, weight in token_weights(escape_important(text), 1.0):
            for word in unescape_important(segment).replace("\n", " ").split(" "):
                if word == "":
                    continue
                if word.startswith(self.embedding_identifier):
                    name = word[len(self.embedding_identifier):].strip("\n")
                    embed, leftover = self._try_get_embedding(name)
                    if embed is not None:
                        if embed.dim() == 1:
                            tokens.append([(embed, weight)])
                        else:
                            tokens.append([(embed[i], weight) for i in range(embed.shape[0])])
                    if leftover == "":
                        continue
                    word = leftover
                tokens.append([(t, weight) for t in bpe.encode(word)])
        batched, batch = [], [(start, 1.0, 0)]
        batched.append(batch)
        for i, group in enumerate(tokens):
            is_large = len(group) >= self.max_word_length
            while len(group) > 0:
                if len(group) + len(batch) > self.max_length - 1:
                    remaining = self.max_length - len(batch) - 1
                    if is_large:
                        batch.extend([(t, w, i + 1) for t, w in group[:remaining]])
                        batch.append((end, 1.0, 0))
                        group = group[remaining:]
                    else:
                        batch.append((end, 1.0, 0))
                        if self.pad_to_max_length:
                            batch.extend([(pad, 1.0, 0)] * remaining)
                    batch = [(start, 1.0, 0)]
                    batched.append(batch)
                else:
                    batch.extend([(t, w, i + 1) for t, w in group])
                    group = []
        batch.append((end, 1.0, 0))
        if self.pad_to_max_length:
            batch.extend([(pad, 1.0, 0)] * (self.max_length - len(batch)))
        if self.min_length is not None and len(batch) < self.min_length:
            batch.extend([(pad, 1.0, 0)] * (self.min_length - len(batch)))
        if not return_word_ids:
            batched = [[(t, w) for t, w, _ in x] for x in batched]
        return batched

    def untokenize(self, pairs):
        return [(a, self.bpe.decoder[a[0]]) for a in pairs]


@functools.lru_cache(maxsize=4)
def _shared_bpe(path):
    return BPE(path)


class SD1Tokenizer:
    def __init__(self, clip_name="l", tokenizer=None, merges_path=None):
        self.clip_name, self.clip = clip_name, "clip_" + clip_name
        setattr(self, self.clip, tokenizer or SDTokenizer(merges_path=merges_path))

    def tokenize_with_weights(self, text, return_word_ids=False):
        return {self.clip_name: getattr(self, self.clip).tokenize_with_weights(text, return_word_ids)}

    def untokenize(self, pairs):
        return getattr(self, self.clip).untokenize(pairs)


def clip_g_tokenizer(merges_path=None):
    """sdxl_clip.SDXLClipGTokenizer: pad 0, 1280-wide embeddings under the key clip_g"""
    return SDTokenizer(pad_with_end=False, embedding_size=1280, embedding_key="clip_g", merges_path=merges_path)


class SDXLTokenizer:
    def __init__(self, merges_path=None):
        self.clip_l = SDTokenizer(merges_path=merges_path)
        self.clip_g = clip_g_tokenizer(merges_path)

    def tokenize_with_weights(self, text, return_word_ids=False):
        return {"g": self.clip_g.tokenize_with_weights(text, return_word_ids), "l": self.clip_l.tokenize_with_weights(text, return_word_ids)}

    def untokenize(self, pairs):
        return self.clip_g.untokenize(pairs)

