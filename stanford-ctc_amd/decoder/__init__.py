"""Drop-in for the reference's ``ctc_fast/decoder/`` directory: the lexicon-constrained
word-bigram prefix beam search (``bg_decoder.decode_bg_lm``), its prefix tree and its LM,
decoding on the MI355X through libsctc_hip.so."""
