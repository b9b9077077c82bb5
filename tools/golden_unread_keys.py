#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""
Audit of what the golden fixtures pin: for every ``tests/golden/golden_*.npz``, the keys that never appear in ``tests/*.py``.
A fixture array that no test reads is a pin that holds nothing.

A key counts as read when the text of some ``tests/*.py`` contains it with case ignored and every run of index digits allowed
to be a number or a ``{...}`` replacement field, so ``case3_flux`` is found in ``f'case{i}_flux'``.  Keys found only in pieces
-- cut at underscores, each piece quoted or next to a replacement field, as in ``GOLDEN[key + '_times']`` or
``for key in ('mean_flux', ...): g[f'case{i}_{key}']`` -- are listed apart as "in pieces"; so are keys that a test reaches by
a quoted prefix (``k.startswith('cat_')``).  What remains is "unread": nothing in the tests names it.

    python tools/golden_unread_keys.py            # prints one line per fixture and group of keys
"""
import glob
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = r'(?:\d+|\{[^{}]*\})'


def pattern(key):
	"""Regex of ``key`` with every digit run generalised to a number or a replacement field."""
	return ''.join(FIELD if part.isdigit() else re.escape(part) for part in re.split(r'(\d+)', key.lower()) if part)


def in_pieces(key, text):
	"""True if ``key`` can be cut at underscores into pieces that each stand in the text between a quote or a replacement field
	on either side (an underscore may stay with the neighbour): ``key + '_times'``, ``f'case{i}_{key}'`` with ``'mean_flux'``."""
	tokens = key.lower().split('_')
	n = len(tokens)
	found = {}

	def piece(i, j):
		if (i, j) not in found:
			found[i, j] = re.search(r"""(?:['"]|\})_?""" + pattern('_'.join(tokens[i:j])) + r"""_?(?:['"]|\{)""", text) is not None
		return found[i, j]
	reach = [True] + [False] * n
	for j in range(1, n + 1):
		reach[j] = any(reach[i] and piece(i, j) for i in range(j))
	return reach[n]


def classify(key, text):
	if re.search(r'(?<![a-z0-9_])' + pattern(key) + r'(?![a-z0-9_])', text):
		return 'read'
	if in_pieces(key, text):
		return 'in pieces'
	# by prefix: startswith('cat_'), startswith(f'c{c}_in_')
	for q in re.findall(r"""startswith\(\s*f?['"]([^'"]+)['"]""", text):
		q = ''.join(r'\d+' if part.startswith('{') else re.escape(part) for part in re.split(r'(\{[^{}]*\})', q) if part)
		if re.match(q, key.lower()):
			return 'by prefix'
	return 'unread'


def generalise(key):
	return re.sub(r'\d+', '#', key)


def main():
	text = '\n'.join(open(p, encoding='utf-8').read() for p in sorted(glob.glob(os.path.join(ROOT, 'tests', '*.py')))).lower()
	unread_total = 0
	for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'golden_*.npz'))):
		with np.load(path, allow_pickle=False) as g:
			keys = list(g.files)
		groups = {}
		for k in keys:
			groups.setdefault((classify(k, text), generalise(k)), []).append(k)
		line = [f"{os.path.basename(path)}: {len(keys)} keys"]
		for kind in ('unread', 'in pieces', 'by prefix'):
			names = sorted(f"{g} (x{len(v)})" if len(v) > 1 else g for (c, g), v in groups.items() if c == kind)
			if names:
				line.append(f"  {kind}: " + ', '.join(names))
			if kind == 'unread':
				unread_total += sum(len(v) for (c, g), v in groups.items() if c == kind)
		print('\n'.join(line))
	print(f"{unread_total} unread keys")
	return 0


if __name__ == '__main__':
	sys.exit(main())
