"""Sites as ranks: process group, aggregation engines, low-rank numerics."""
from .group import SiteGroup, current, init_sites, shutdown
from .engines import (DSGDEngine, Engine, FedAvgEngine, PowerSGDEngine, RankDADEngine, TopKEngine,
                      TrimmedMeanEngine, ENGINES, make_engine)
from . import privacy

__all__ = ["SiteGroup", "current", "init_sites", "shutdown", "Engine", "DSGDEngine",
           "RankDADEngine", "PowerSGDEngine", "TopKEngine", "TrimmedMeanEngine", "FedAvgEngine",
           "ENGINES", "make_engine", "privacy"]
