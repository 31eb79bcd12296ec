"""The small helpers of the reference's ``decoder/decoder_utils.py``, with paths as arguments
where the reference reads a site configuration."""


def load_chars(char_file):
    """``token id`` per line -> {token: symbol id}"""
    with open(char_file) as f:
        pairs = [l.split() for l in f if l.strip()]
    return dict((p[0], int(p[1])) for p in pairs)


def load_words(word_file):
    """one word per line"""
    with open(word_file) as f:
        return [l.strip() for l in f if l.strip()]


def int_to_char(int_seq, char_map):
    """symbol ids -> tokens; char_map: {token: symbol id}"""
    inv = dict((v, k) for k, v in char_map.items())
    return [inv[int(i)] for i in int_seq]


def collapse_seq(char_seq, space="[space]"):
    """tokens -> the sentence: the space token becomes ' ', everything else is joined"""
    return "".join(" " if c == space else c for c in char_seq)
