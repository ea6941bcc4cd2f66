"""pingoo_amd — MI355X-native batched WAF rule matching for Pingoo's per-request rule path."""
from . import _abi  # noqa: F401
from .batch import GEO_DTYPE, GEOIP_DTYPE, RESPONSE_DTYPE, RULE_HIT_DTYPE, VERDICT_DTYPE, Request, RequestBatch, geoip_entries, hits_to_matrix  # noqa: F401
from .engine import KeySet, client_ids, derive_batch, derive_stats, generate_captcha_client_id, verify_cookie, verify_cookies, pow_handed, verify_pow, verify_pow_one, body_column, body_stats, parse_pow_bodies, parse_pow_body_one, respond, respond_one, respond_scan_shape  # noqa: F401,E402
