"""CPU: the table of tests/graph_forms.py against include/spfe.h.  Every declared function whose name ends in _device has an
entry — spfe_extract_batch_device alone is excused, tools/graph_capture_check.py captures it through tests/test_gpu_parity.py —,
so a form added later fails here until it has one; every entry names a declared form; and the sentence an entry quotes for its
launch count still stands in the header (comment stars and line breaks apart)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_forms  # noqa: E402

EXCUSED = {"extract_batch"}


def header():
    with open(os.path.join(ROOT, "include", "spfe.h")) as f:
        return f.read()


def declared_device_forms(text):
    return set(re.findall(r"\bSPFE_API\s+[A-Za-z_ ]*?\bspfe_(\w+)_device\s*\(", text))


def flat(text):
    """the header as running text: the stars that open comment lines and all white space collapsed"""
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*\s?", "\n", text))


def test_every_device_form_of_the_header_is_in_the_table():
    forms = declared_device_forms(header())
    assert len(forms) == 37 and EXCUSED <= forms, sorted(forms)
    assert forms - EXCUSED == set(graph_forms.FORMS), (sorted(forms - EXCUSED - set(graph_forms.FORMS)),
                                                      sorted(set(graph_forms.FORMS) - forms))


def test_the_parser_sees_a_form_that_has_no_entry():
    text = header() + "\nSPFE_API int spfe_something_new_device(spfe_handle h, void *stream);\n"
    assert declared_device_forms(text) - EXCUSED - set(graph_forms.FORMS) == {"something_new"}


def test_every_quoted_sentence_stands_in_the_header():
    text = flat(header())
    for name, form in graph_forms.FORMS.items():
        assert flat(form.sentence) in text, (name, form.sentence)
        assert form.kernels is not None and form.kernels >= 1 and form.memsets >= 0, name
        if form.stated:                                  # the sentence states the number: as a word or as ONE
            words = {1: ("one ", "ONE "), 2: ("two ", "Two "), 3: ("three ", "Three ")}[form.kernels]
            assert any(w in form.sentence or w.capitalize() in form.sentence for w in words), (name, form.kernels, form.sentence)
