"""Drop-in for the reference's ``ctc_fast/new_decoder`` package (decoder.pyx)."""
