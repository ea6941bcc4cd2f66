"""TEST-ONLY: table_walker.Tables for a program compiled with routes (pwaf_program_compile_routed). Reads the dump's route section
and answers (action, rule_idx, route) per request: the verdict as Tables.evaluate gives it over ALL device rules (a route has both
effects 0 and never decides), the route as the first device rule of the route range whose literal lists hold. Shared by the CPU and
GPU route tests, with the two oracle constructions they compare against."""
from __future__ import annotations

import struct

import numpy as np

from oracle import pyoracle
from pingoo_amd import _abi
from table_walker import Tables, parse_dump

NO_GATES = _abi.OPT_NO_UA_GATE | _abi.OPT_NO_CAPTCHA_BYPASS


class RoutedTables(Tables):
    def __init__(self, blob):
        raw = blob.dump() if hasattr(blob, "dump") else blob
        super().__init__(blob)
        self.route_base, self.n_dev_routes, self.n_routes, self.n_user_rules = self.n_rules, 0, 0, None
        for tag, count, pl in parse_dump(raw):
            if tag == "ROUT":
                assert count == 4
                self.route_base, self.n_dev_routes, self.n_routes, self.n_user_rules = struct.unpack("<4I", pl)
        assert self.route_base + self.n_dev_routes == len(self.rules)
        mine = self.rules[self.route_base:]
        assert (mine["eff_u"] == 0).all() and (mine["eff_v"] == 0).all() and (np.diff(mine["public_idx"].astype(np.int64)) > 0).all()
        assert len(mine) == 0 or int(mine["public_idx"][-1]) < self.n_routes

    def evaluate_routed(self, batch, i: int):
        action, rule = Tables.evaluate(self, batch, i)
        every = self.rules
        routes = every[self.route_base:].copy()
        routes["eff_u"] = routes["eff_v"] = _abi.ACTION_BLOCK  # (first match wins over the route range alone)
        self.rules = routes
        try:
            a, k = Tables.evaluate(self, batch, i)
        finally:
            self.rules = every
        return action, rule, (int(k) if a else -1)


def oracle_verdicts(rules, lists, geo, batch, flags=0):
    return pyoracle.Oracle(rules, lists, geo, flags=flags).evaluate(batch)


def oracle_routes(routes, lists, geo, batch) -> np.ndarray:
    """tests/test_gpu_paths.py::test_service_routing_is_first_match_over_route_expressions: route k 'blocks' with rule index k, no gate"""
    want = pyoracle.Oracle([(n, e, [_abi.RULE_ACTION_BLOCK]) for n, e in routes], lists, geo, flags=NO_GATES).evaluate(batch)
    return np.where(want["action"] == _abi.ACTION_BLOCK, want["rule_idx"].astype(np.int64), -1).astype(np.int32)


HEADERS = ["x-a", "cookie", "referer"]
# never true (no generated value holds a '~'); names every header of helpers.lit_pred in one order. Put first among the rules AND among
# the routes, it gives the engine (names collected over the rules, then the routes) and both oracles the same header columns.
NAMES_EXPR = " && ".join(f'http_request.headers["{h}"] == "~~"' for h in HEADERS)


def split(exprs, n_rules, rng, actions):
    """a generated list of expressions -> (rules, routes): the first n_rules become rules, the rest routes"""
    rules = [(f"r{k}", e, actions(rng)) for k, e in enumerate(exprs[:n_rules])]
    routes = [(f"s{k}", e) for k, e in enumerate(exprs[n_rules:])]
    return rules, routes
