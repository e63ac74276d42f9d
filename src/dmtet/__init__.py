"""src.dmtet: this project provides geometry.dmtet_geometry; the rest (render, ...) falls through to the next
``src`` tree on sys.path."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
