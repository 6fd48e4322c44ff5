# -*- coding: utf-8 -*-
"""Synonym extraction from dependency triples (reference east/synonyms/)."""
from east.synonyms.synonyms import SynonymExtractor  # noqa: F401
