"""The sharded plaid.test engine (shard_plaid_test.cpp) with `nshards` contexts on one device, through the library's test hook."""
from tests.helpers.sharded_hooks import plaid_test as run  # noqa: F401
