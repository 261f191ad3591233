"""Inputs of the TEXT tests, rebuilt from short recipes: tests/golden/text.json stores the recipes and what the reference computed from
them (tools/make_text_golden.py), the tests rebuild the bytes. A recipe is [kind, size, seed, ...]; a stage case is (name, recipe, data
type the block comes with). Every case runs for the three codecs (1: FPAQ, 2: ANS0, 3: TPAQX) and the stream block sizes BLOCK_SIZES."""
import numpy as np

CHUNK = 4096           # positions per workgroup of the device stage (text.hip: TX_CHUNK)
WINDOW = 64            # words per step of the dictionary walk
BLOCK_SIZES = (0, 65536, 4 << 20)
ENTROPY = {1: "FPAQ", 2: "ANS0", 3: "TPAQX"}
ENTROPY_ID = {1: 2, 2: 5, 3: 9}
H1, H2 = 0x7FEB352D, 0x846CA68B
STATIC = [b"the", b"and", b"that", b"with", b"have", b"would", b"because", b"through", b"which", b"their", b"there", b"could"]


def word_hash(w):
    h = H1
    for c in w:
        h = ((h * H1) ^ (c * H2)) & 0xFFFFFFFF
    return h


def _pool(rng, count, lo=2, hi=10):
    return [rng.integers(97, 123, int(rng.integers(lo, hi)), dtype=np.uint8).tobytes() for _ in range(count)]


def plain(n, seed, newline=b"\n"):
    """Words of a pool of 300 and static words, some capitalised, separated by spaces, punctuation and line ends"""
    rng = np.random.default_rng(seed)
    pool = _pool(rng, 300) + STATIC
    out = bytearray()
    while len(out) < n:
        w = pool[int(rng.integers(0, len(pool)))]
        if rng.random() < 0.15:
            w = w[:1].upper() + w[1:]
        r = rng.random()
        out += w + (b" " if r < 0.8 else b", " if r < 0.88 else b". " if r < 0.94 else newline)
    return bytes(out[:n])


def counted_words(first, count, letters):
    """`count` distinct words of `letters` letters: the numbers from `first` in base 26"""
    v = np.arange(first, first + count, dtype=np.int64)
    cols = []
    for _ in range(letters):
        cols.append((v % 26 + 97).astype(np.uint8))
        v //= 26
    cols.append(np.full(count, 32, dtype=np.uint8))
    return np.stack(cols, axis=1).tobytes()


def colliding_pair(seed, bits=13):
    """Two different five-letter words whose hashes share a slot of a map of 2^bits slots, neither one a slot of a static word"""
    rng = np.random.default_rng(seed)
    seen = {}
    taken = {word_hash(w) & ((1 << bits) - 1) for w in STATIC}
    while True:
        w = rng.integers(97, 123, 5, dtype=np.uint8).tobytes()
        s = word_hash(w) & ((1 << bits) - 1)
        if s in taken or s == 0:
            continue
        if s in seen and seen[s] != w:
            return seen[s], w
        seen[s] = w


def make(recipe):
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    rng = np.random.default_rng(seed + 1000)
    if kind == "plain":
        return plain(n, seed)
    if kind == "lead":
        return (b" " * recipe[3] + plain(n, seed))[:n]
    if kind == "crlf":
        d = plain(n + 64, seed, b"\r\n")
        d = d[:n - 2].rstrip(b"\r") + b"\r\n"
        d = d + b"x" * (n - len(d))
        if recipe[3]:                                               # one bare line feed
            at = d.index(b"\r\n", n // 2)
            d = d[:at] + b" \n" + d[at + 2:]
        return d
    if kind == "xml":
        out = bytearray()
        body = plain(n, seed).split(b" ")
        k = 0
        while len(out) < n:
            out += b"<item id=\"%d\">" % k + b" ".join(body[k % 200:k % 200 + 8]) + b" &amp; &lt;b&gt; &quot;x&quot;</item>\n"
            k += 1
        return bytes(out[:n])
    if kind == "esc":
        d = bytearray(plain(n, seed))
        for k, at in enumerate(rng.choice(n, 40, replace=False)):
            d[at] = 0x0E + (k & 1)
        return bytes(d)
    if kind == "high":                                              # recipe[3] bytes of 0x80 and above, evenly spread
        d = bytearray(plain(n, seed))
        for at in np.linspace(0, n - 1, recipe[3]).astype(np.int64):
            d[at] = 0xE9
        assert sum(c >= 128 for c in d) == recipe[3]
        return bytes(d)
    if kind == "magic":
        return b"\x89PNG" + plain(n - 4, seed)
    if kind == "dna":
        d = np.array(list(b"ACGT"), dtype=np.uint8)[rng.integers(0, 4, n)]
        d[60::61] = 10
        return d.tobytes()
    if kind == "numeric":
        return np.array(list(b"0123456789+-*/=,.:; "), dtype=np.uint8)[rng.integers(0, 20, n)].tobytes()
    if kind == "base64":
        return np.array(list(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"), dtype=np.uint8)[rng.integers(0, 64, n)].tobytes()
    if kind == "bin":
        return rng.permutation(np.arange(n, dtype=np.int64) % 256).astype(np.uint8).tobytes()
    if kind == "small":
        return np.array(list(b"01#%"), dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    if kind == "utf8":
        words = ["слово", "текст", "пример", "данные", "и", "в"]
        out = []
        while sum(len(w) + 1 for w in out) * 2 < n + 32:
            out.append(words[int(rng.integers(0, len(words)))])
        d = " ".join(out).encode("utf-8")[:n]
        while (d[-1] & 0xC0) == 0x80 or d[-1] >= 0xC0:              # (no sequence is cut at the end)
            d = d[:-1]
        return d + b" " * (n - len(d))
    if kind == "undef":
        return rng.integers(0, 200, n, dtype=np.uint8).tobytes()
    if kind == "wordlens":                                          # words of 2, 3, 31 and 32 letters, each of them several times
        special = [b"qz", b"qzx", b"q" * 15 + b"z" * 16, b"q" * 16 + b"z" * 16]
        body = plain(n, seed).split(b" ")
        out = bytearray()
        k = 0
        while len(out) < n:
            out += body[k % len(body)] + b" " + special[k % 4] + b" "
            k += 1
        return bytes(out[:n])
    if kind == "static":                                            # static words, as they are and with the first letter's case flipped
        out = bytearray()
        k = 0
        while len(out) < n:
            w = STATIC[int(rng.integers(0, len(STATIC)))]
            out += (w[:1].upper() + w[1:] if k % 3 == 1 else w) + (b" " if k % 7 else b".\n")
            k += 1
        return bytes(out[:n])
    if kind == "twice":                                             # a new word twice within a window, and next to its case flip
        out = bytearray()
        k = 0
        while len(out) < n:
            w = counted_words(1000 + k, 1, 6)[:6]
            out += w + b" " + w + b" " + w[:1].upper() + w[1:] + b" the " + w[:1].upper() + w[1:] + b"\n"
            k += 1
        return bytes(out[:n])
    if kind == "collide":                                           # two new words that share a slot, recipe[3] words apart
        a, b = colliding_pair(seed)
        gap = b" ".join(STATIC[k % len(STATIC)] for k in range(recipe[3]))
        head = a + b" " + gap + b" " + b + b" " + a + b" " + b + b" " + gap + b" " + b + b" " + a + b"\n"
        return (head + plain(n, seed))[:n]
    if kind == "distinct":                                          # distinct words, so the dictionary grows; the last third repeats them
        first = counted_words(0, n // 9 + 1, 5)
        return (first + first)[:n]
    if kind == "grow3":
        # more than 16,384 entries, then new three-letter words (no longer taken) and repeats of early and late words (indexes of 1, 2
        # and 3 bytes in both codecs)
        first = counted_words(0, 17000, 5)
        three = counted_words(0, 2000, 3)
        rep = b"".join(counted_words(int(v), 1, 5) for v in rng.integers(0, 17000, 6000))
        few = b"".join(counted_words(int(v), 1, 5) for v in rng.integers(0, 40, 2000))
        d = first + three + rep + few + three
        return (d + plain(n, seed))[:n]
    if kind == "wrap":
        # more than 2^19 entries, so the index wraps and entries are replaced; then early words (gone), late words and new ones
        first = counted_words(0, 530000, 5)
        late = counted_words(400000, 20000, 5)
        early = counted_words(0, 20000, 5)
        d = first + late + early + late
        return (d + plain(n, seed))[:n]
    if kind == "overflow":                                          # escapes make the output outgrow the block midway
        d = np.frombuffer(plain(n, seed), dtype=np.uint8).copy()
        d[n // 8:][rng.random(n - n // 8) < 0.6] = 0x0F
        return d.tobytes()
    raise ValueError(kind)


def stage_cases():
    cases = [
        ("plain 1023", ["plain", 1023, 1], 0),
        ("plain 1024", ["plain", 1024, 1], 0),
        ("plain 9000", ["plain", 2 * CHUNK + 808, 2], 0),
        ("plain 4096", ["plain", CHUNK, 3], 0),
        ("leading spaces", ["lead", 5000, 4, 70], 0),
        ("crlf", ["crlf", 6000, 5, 0], 0),
        ("crlf with a bare lf", ["crlf", 6000, 5, 1], 0),
        ("xml", ["xml", 9000, 6], 0),
        ("escape bytes", ["esc", 5000, 7], 0),
        ("high bytes just under a quarter", ["high", 8192, 8, 2048], 0),
        ("high bytes just over a quarter", ["high", 8192, 8, 2049], 0),
        ("magic", ["magic", 3000, 9], 0),
        ("dna", ["dna", 3000, 10], 0),
        ("numeric", ["numeric", 3000, 11], 0),
        ("base64", ["base64", 3000, 12], 0),
        ("bin", ["bin", 4096, 13], 0),
        ("small alphabet", ["small", 3000, 14], 0),
        ("utf8", ["utf8", 3000, 15], 0),
        ("undefined", ["undef", 3000, 16], 0),
        ("word lengths", ["wordlens", 6000, 17], 0),
        ("static words", ["static", 3000, 18], 0),
        ("new word twice", ["twice", 3000, 19], 0),
        ("colliding words in a window", ["collide", 3000, 20, 3], 0),
        ("colliding words across windows", ["collide", 4000, 20, 3 * WINDOW], 0),
        ("distinct words 128 KiB", ["distinct", 128 * 1024 + 77, 21], 0),
        ("three letters behind 16384 entries", ["grow3", 205000, 22], 0),
        ("wrap 4 MiB", ["wrap", 4 << 20, 23], 0),
        ("overflow", ["overflow", 6000, 24], 0),
    ]
    cases += [("preset %d" % dt, ["plain", 2048, 30], dt) for dt in range(1, 10)]
    return cases


def damage(enc, op, codec):
    """A damaged copy of an encoded block. op: [kind, ...]"""
    d = bytearray(enc)
    kind = op[0]
    if kind == "cut":                                               # the block ends inside the first multi-byte index
        for i in range(1, len(d) - 2):
            if codec != 2 and d[i] in (0x0E, 0x0F) and d[i + 1] >= 0x80:
                return bytes(d[:i + 2])
            if codec == 2 and d[i] >= 0xC0 and d[i - 1] != 0x0F:
                return bytes(d[:i + 1])
        return bytes(d[:len(d) - 1])
    if kind == "append":                                            # bytes behind the block
        return bytes(d) + bytes(op[1])
    raise ValueError(kind)


def damaged_cases(codec):
    """(name, op) of the damaged blocks, each applied to the output of "plain 9000" """
    big1, big2 = bytes([0x0F, 0xFF, 0xFF, 0x7F]), bytes([0xFF, 0xFF, 0xFF])
    cases = [("cut inside an index", ["cut"])]
    if codec != 2:
        cases += [("index beyond the dictionary", ["append", list(big1)]),
                  ("unused entry", ["append", [0x20, 0x0F, 0xBF, 0x7F]])]          # entry 8191: no word of a block this short reaches it
    else:
        cases += [("index beyond the dictionary", ["append", list(big2)]),
                  ("index 0 in two bytes", ["append", [0x20, 0xC0, 0x00]]),
                  ("index 0 in three bytes", ["append", [0x20, 0xF0, 0x00, 0x00]]),
                  ("unused entry", ["append", [0x20, 0xDF, 0xFF]])]                  # entry 8190
    return cases


DAMAGE_FROM = "plain 9000"

# streams against the reference's: 300,000 bytes of text in blocks of 64 KiB
STREAM = ["plain", 300000, 40]
STREAM_BS = 65536
STREAM_BLOCKS = 5
STREAM_CHAINS = [
    ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 32),
    ("TEXT+UTF+BWT+SRT+ZRLT", "FPAQ", 0),
    ("LZP+TEXT+UTF+BWT+LZP", "CM", 64),
    ("ZRLT+TEXT", "HUFFMAN", 0),
    ("PACK+TEXT", "ANS0", 0),
    ("MM+TEXT", "FPAQ", 0),
    ("UTF+TEXT", "RANGE", 0),
    ("ROLZX+TEXT", "NONE", 0),
    ("EXE+TEXT", "TPAQ", 0),
    ("RLT+TEXT+UTF", "TPAQX", 0),
    ("TEXT+RLT", "HUFFMAN", 0),
    ("EXE+RLT+TEXT+UTF+DNA", "TPAQ", 0),
    ("EXE+RLT+TEXT+UTF+DNA", "TPAQX", 32),
]
# DNA (PACK that takes DNA blocks only): an ACGT block, which it takes, and a text block, which it refuses
DNA_KINDS = [["dna", 65536, 60], ["plain", 65536, 61]]
DNA_CHAINS = [("DNA+RLT", "HUFFMAN", 0), ("DNA", "NONE", 32)]
# streams of 4 MiB blocks (hash maps of 2^19 and 2^17 slots; TPAQX, 2^20, codes a block of this size too slowly for a test): the block that wraps the index and the one that passes 16,384 entries
BIG_KINDS = [["wrap", 4 << 20, 23], ["grow3", 205000, 22]]
BIG_BS = 4 << 20
BIG_CHAINS = [("TEXT", "FPAQ", 0), ("TEXT", "NONE", 0)]
# eight blocks of 64 KiB of different kinds in one batch
MIXED_KINDS = [["plain", 65536, 50], ["crlf", 65536, 51, 0], ["xml", 65536, 52], ["dna", 65536, 53], ["bin", 65536, 54], ["utf8", 65536, 55],
               ["esc", 65536, 56], ["distinct", 65536, 57]]
MIXED_CHAINS = [("TEXT", "NONE", 0), ("TEXT", "FPAQ", 32)]


def mixed():
    return b"".join(make(r) for r in MIXED_KINDS)


def dna_blocks():
    return b"".join(make(r) for r in DNA_KINDS)


def big_blocks():
    return b"".join(make(r) for r in BIG_KINDS)

# levels of the command-line tool whose chains have TEXT behind a device stage
CLI_LEVELS = [7, 8, 9]
