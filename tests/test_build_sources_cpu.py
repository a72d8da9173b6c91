"""build.SOURCES against the translation units on disk: a unit that is forgotten, or deleted but still listed, fails here and not at
link time on the GPU machine."""
import os

from deepctr_amd import build


def test_sources_has_no_duplicates():
    assert len(build.SOURCES) == len(set(build.SOURCES))


def test_sources_is_every_translation_unit_of_csrc():
    on_disk = {f for f in os.listdir(build.SRC) if f.endswith((".hip", ".cpp"))}
    assert set(build.SOURCES) == on_disk
