"""CLIP's byte-pair tokenizer: what `clip.tokenize(text)` (clip_fft.py:119 and every place a prompt is encoded) computes, restated from
openai/CLIP's clip/simple_tokenizer.py.

    tok = Tokenizer('/path/bpe_simple_vocab_16e6.txt.gz', vocab_size=49408)
    ids = tok.tokenize(['a photo of a cat'])            # int32 [1, 77]: SOT, ids, EOT, zero padding

The vocabulary file is the user's, like the checkpoint: upstream's bpe_simple_vocab_16e6.txt.gz, the same text unpacked, or a HuggingFace
merges.txt -- one header line, then one merge ("left right") per line.  The first vocab_size - 512 - 2 merges are used.

One step of upstream is NOT taken: `ftfy.fix_text` (mojibake repair) -- ftfy is not a dependency here.  Text that is already proper
Unicode, which is what a command line hands over, tokenizes identically.
"""
import gzip
import html

import regex
import torch

SOT, EOT = '<|startoftext|>', '<|endoftext|>'
_PIECES = regex.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+", regex.IGNORECASE)


def byte_symbols():
    """GPT-2's byte -> printable unicode character table, in id order: the printable Latin-1 bytes stand for themselves, the other 68 are
    mapped to U+0100 ... in byte order"""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    rest = [b for b in range(256) if b not in keep]
    table = {b: chr(b) for b in keep}
    table.update({b: chr(256 + n) for n, b in enumerate(rest)})
    return table            # (dicts keep insertion order: keep, then rest -- the order of the first 256 ids)


def read_merges(path, count):
    """the first `count` merges of a vocabulary file (gzip or plain text; the first line is a header)"""
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:2] == b'\x1f\x8b':
        raw = gzip.decompress(raw)
    lines = raw.decode('utf-8').split('\n')[1:]
    merges = [tuple(ln.split()) for ln in lines[:count] if ln.strip()]
    if len(merges) < count or any(len(m) != 2 for m in merges):
        raise ValueError('%s holds %d usable merges; a vocabulary of %d entries needs %d (512 byte symbols + merges + 2 markers)'
                         % (path, len(merges), count + 514, count))
    return merges


def clean(text):
    """upstream's basic_clean (without ftfy) + whitespace_clean + lower()"""
    text = html.unescape(html.unescape(text)).strip()
    return regex.sub(r'\s+', ' ', text).strip().lower()


class Tokenizer:
    def __init__(self, bpe_path, vocab_size=49408):
        if vocab_size < 514:
            raise ValueError('vocab_size %d: a CLIP vocabulary has at least 512 byte symbols and 2 markers' % vocab_size)
        self.byte_symbol = byte_symbols()
        merges = read_merges(bpe_path, vocab_size - 512 - 2)
        symbols = list(self.byte_symbol.values())
        vocab = symbols + [s + '</w>' for s in symbols] + [a + b for a, b in merges] + [SOT, EOT]
        self.encoder = {s: i for i, s in enumerate(vocab)}
        self.rank = {m: i for i, m in enumerate(merges)}
        self.vocab_size = vocab_size
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]
        self._cache = {SOT: (SOT,), EOT: (EOT,)}

    def bpe(self, piece):
        """a piece (byte symbols) -> its BPE symbols: repeatedly merge the adjacent pair of lowest rank, every occurrence left to right"""
        if piece in self._cache:
            return self._cache[piece]
        word = list(piece[:-1]) + [piece[-1] + '</w>']
        while len(word) > 1:
            pairs = set(zip(word, word[1:]))
            best = min(pairs, key=lambda p: self.rank.get(p, float('inf')))
            if best not in self.rank:
                break
            out, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and (word[i], word[i + 1]) == best:
                    out.append(word[i] + word[i + 1])
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = out
        self._cache[piece] = tuple(word)
        return self._cache[piece]

    def encode(self, text):
        ids = []
        for piece in _PIECES.findall(clean(text)):
            piece = ''.join(self.byte_symbol[b] for b in piece.encode('utf-8'))
            ids.extend(self.encoder[s] for s in self.bpe(piece))
        return ids

    def tokenize(self, texts, context_length=77, truncate=False):
        """str or list of str -> int32 [n, context_length]: SOT + ids + EOT, zero padded.  A text that does not fit raises RuntimeError;
        with truncate=True it is cut and its last id set to EOT."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.int32)
        for i, text in enumerate(texts):
            ids = [self.sot] + self.encode(text) + [self.eot]
            if len(ids) > context_length:
                if not truncate:
                    raise RuntimeError('Input %s is too long for context length %d' % (text, context_length))
                ids = ids[:context_length]
                ids[-1] = self.eot
            out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return out
