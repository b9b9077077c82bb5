# -*- coding: utf-8 -*-
"""Counting the allocations of a context at the C entries: what the loaders' tests hold their "after any exception everything is gone" to."""


def count_allocations(ctx, monkeypatch):
	"""
	Wrap ``tp_malloc`` / ``tp_free`` / ``tp_host_alloc`` / ``tp_host_free`` of ``ctx.lib`` (undone with ``monkeypatch``).  Returns the dict
	``{'device': n, 'host': n}`` of the blocks, device and page-locked, that live on ``ctx.handle``; other contexts are not counted.
	"""
	live = {'device': 0, 'host': 0}
	lib = ctx.lib
	calls = {name: getattr(lib, name) for name in ('tp_malloc', 'tp_free', 'tp_host_alloc', 'tp_host_free')}

	def counting(name, kind, step):
		def call(handle, *args):
			rc = calls[name](handle, *args)
			if rc == 0 and handle == ctx.handle:
				live[kind] += step
			return rc
		return call
	for name, kind, step in (('tp_malloc', 'device', 1), ('tp_free', 'device', -1), ('tp_host_alloc', 'host', 1), ('tp_host_free', 'host', -1)):
		monkeypatch.setattr(lib, name, counting(name, kind, step))
	return live
